// journal_refusals.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_update_journaled_device_into and
// p252_merkle{4,2}_forest_ragged_journal_swap_device_into, as a table in the format and by the method of api_refusals.cpp
// (refusal_table.hpp holds the harness):
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so ONE context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  For each entry point the control row — an all-good argument set — must get past validation and fail
// at hipSetDevice(ctx->device) with P252_ERR_HIP; every other row varies one argument (ctx NULL, every pointer NULL, every aligned
// array off by half its alignment, every count at 0 and at both sides of every size check, the journal's capacity at both sides of the
// call's bound) or a named combination.  No pointer is dereferenced: no row reaches a device.
// (tests/test_forest_journal_cpu.py compares the lines with tests/golden/journal_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

std::vector<Entry> entries() {
    std::vector<Entry> es;
    for (unsigned arity : {4u, 2u}) {
        const bool a4 = arity == 4;
        {
            // the journal's bound for the control row's sizes (n_leaves 12, n_trees 3, max_leaves 5, k 7): 7 + min(7, 12 / A^l + 3) per level
            const uint64_t jbound = a4 ? 7 + 6 + 3 : 7 + 7 + 6 + 4;
            std::vector<Combo> cs = forest_shape_combos();
            cs.push_back({"k=SIZE_MAX/128", {{"k", MAXZ / 128}}});
            cs.push_back({"k=SIZE_MAX/128+1", {{"k", MAXZ / 128 + 1}}});
            cs.push_back({"max_leaves=1,d_levels=NULL", {{"max_leaves", 1}, {"d_levels", 0}}});
            cs.push_back({"max_leaves=1,journal_cap=7", {{"max_leaves", 1}, {"journal_cap", 7}}});
            cs.push_back({"max_leaves=1,journal_cap=6", {{"max_leaves", 1}, {"journal_cap", 6}}});
            cs.push_back({"n_leaves=0,k=0", {{"n_leaves", 0}, {"k", 0}}});
            cs.push_back({"k=0,journal_cap=0,d_journal_ids=d_journal_values=NULL", {{"k", 0}, {"journal_cap", 0}, {"d_journal_ids", 0}, {"d_journal_values", 0}}});
            cs.push_back({"k=0,d_journal_len=NULL", {{"k", 0}, {"d_journal_len", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_update_journaled_device_into" : "p252_merkle2_forest_ragged_update_journaled_device_into",
                          {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p4("d_tree_ids"),
                           p8("d_leaf_ids"), p16("d_new_leaves"), cnt("k", 7), p16("d_roots"), p4("d_n_bad"), p8("d_n_hashed"), p16("d_journal_ids"),
                           p16("d_journal_values"), cnt("journal_cap", 40, {jbound - 1, jbound, MAXZ / 64, MAXZ / 64 + 1}), p8("d_journal_len")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_update_journaled_device_into : p252_merkle2_forest_ragged_update_journaled_device_into)(
                                  C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), v[5], v[6], P(v[7]), P(v[8]), P(v[9]), P(v[10]), v[11], P(v[12]), P(v[13]), P(v[14]), P(v[15]),
                                  P(v[16]), v[17], P(v[18]), nullptr);
                          },
                          cs});
            std::vector<Combo> ss = forest_shape_combos();
            ss.push_back({"max_leaves=1,d_levels=NULL", {{"max_leaves", 1}, {"d_levels", 0}}});
            ss.push_back({"n_leaves=1,d_levels=NULL", {{"n_leaves", 1}, {"d_levels", 0}}});
            ss.push_back({"journal_cap=0,every buffer NULL", {{"journal_cap", 0}, {"d_leaves", 0}, {"d_offsets", 0}, {"d_levels", 0}, {"d_journal_ids", 0},
                                                              {"d_journal_values", 0}, {"d_journal_len", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_journal_swap_device_into" : "p252_merkle2_forest_ragged_journal_swap_device_into",
                          {CTXA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p16("d_journal_ids"),
                           p16("d_journal_values"), cnt("journal_cap", 40, {MAXZ / 64, MAXZ / 64 + 1}), p8("d_journal_len"), p16("d_roots"), p4("d_n_bad")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_journal_swap_device_into : p252_merkle2_forest_ragged_journal_swap_device_into)(
                                  C(v[0]), P(v[1]), v[2], P(v[3]), v[4], v[5], P(v[6]), P(v[7]), P(v[8]), v[9], P(v[10]), P(v[11]), P(v[12]), nullptr);
                          },
                          ss});
        }
    }
    return es;
}

}  // namespace

int main() {
    g_ctx = new p252_ctx();  // device = -1: never bound
    for (Entry& e : entries()) run(e);
    delete g_ctx;
    return 0;
}
