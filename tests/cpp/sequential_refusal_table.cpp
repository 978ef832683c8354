// sequential_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_update_sequential_device_into, as a table in the
// format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_sequential_cpu.py compares the lines with tests/golden/sequential_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, d_new_leaves, d_order, k, d_old_leaves,
        d_siblings, d_positions, d_depths, d_roots_before, d_roots_after, d_roots, d_n_bad, d_n_hashed;
};

int update(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_update_sequential_device_into : p252_merkle2_forest_ragged_update_sequential_device_into)(
        a.ctx, a.tag, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_tree_ids), P(a.d_leaf_ids),
        P(a.d_new_leaves), P(a.d_order), a.k, P(a.d_old_leaves), P(a.d_siblings), P(a.d_positions), P(a.d_depths), P(a.d_roots_before),
        P(a.d_roots_after), P(a.d_roots), P(a.d_n_bad), P(a.d_n_hashed), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        // 9 updates of 3 trees of at most 100 of 120 leaves: the witnesses at the stride of 100 leaves (4 or 7 rows), far inside 1 MiB
        const Args good = {ctx,     g_tag,   slot(0), 120,     slot(1), 3,        100,      slot(2),  slot(3),  slot(4),  slot(5),
                           slot(6), 9,       slot(7), slot(8), slot(9), slot(10), slot(11), slot(12), slot(13), slot(14), slot(15)};
        std::vector<Case> cases = {
            {"control", [](Args&) {}},
            {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
            {"tag=NULL", [](Args& a) { a.tag = nullptr; }},
            {"k=0", [](Args& a) { a.k = 0; }},
            {"n_leaves=0", [](Args& a) { a.n_leaves = 0; }},
            {"n_trees=0", [](Args& a) { a.n_trees = 0; }},
            {"max_leaves=0", [](Args& a) { a.max_leaves = 0; }},
            {"k=2^32-1", [](Args& a) { a.k = 0xffffffffull; }},
            {"k=2^32", [](Args& a) { a.k = 1ull << 32; }},
            {"k=SIZE_MAX", [](Args& a) { a.k = MAXZ; }},
            {"max_leaves=2^32-1", [](Args& a) { a.max_leaves = 0xffffffffull; }},
            {"max_leaves=2^32", [](Args& a) { a.max_leaves = 1ull << 32; }},
            {"max_leaves=SIZE_MAX", [](Args& a) { a.max_leaves = MAXZ; }},
            {"optional=NULL", [](Args& a) { a.d_old_leaves = a.d_roots_before = a.d_roots = a.d_n_bad = a.d_n_hashed = 0; }},
            {"max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL",
             [](Args& a) { a.max_leaves = 1, a.d_levels = a.d_siblings = a.d_positions = 0; }},
            {"max_leaves=2,d_levels=NULL", [](Args& a) { a.max_leaves = 2, a.d_levels = 0; }},
            {"max_leaves=2,d_siblings=NULL", [](Args& a) { a.max_leaves = 2, a.d_siblings = 0; }},
            {"max_leaves=2,d_positions=NULL", [](Args& a) { a.max_leaves = 2, a.d_positions = 0; }},
            {"n_leaves=SIZE_MAX/64+1", [](Args& a) { a.n_leaves = MAXZ / 64 + 1; }},
            {"n_trees=SIZE_MAX/8/66+1", [](Args& a) { a.n_trees = TREES_MAX + 1; }},
            {"n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2",
             [](Args& a) { a.n_leaves = 1ull << 40, a.max_leaves = 1ull << 31, a.n_trees = ((MAXZ / 2) >> 31) + 1; }},
            // an output inside an input, inside the forest, inside another output; the forest's own arrays may not hold an output either
            {"d_old_leaves=d_new_leaves", [](Args& a) { a.d_old_leaves = a.d_new_leaves; }},
            {"d_siblings=d_leaves+32", [](Args& a) { a.d_siblings = a.d_leaves + 32; }},
            {"d_roots_after=d_levels", [](Args& a) { a.d_roots_after = a.d_levels; }},
            {"d_roots_before=d_roots", [](Args& a) { a.d_roots_before = a.d_roots; }},
            {"d_depths=d_order+4", [](Args& a) { a.d_depths = a.d_order + 4; }},
            {"d_positions=d_tree_ids", [](Args& a) { a.d_positions = a.d_tree_ids; }},
            {"d_n_bad=d_leaf_ids", [](Args& a) { a.d_n_bad = a.d_leaf_ids; }},
            {"d_n_hashed=d_offsets+8", [](Args& a) { a.d_n_hashed = a.d_offsets + 8; }},
            {"d_roots_after=d_roots_before", [](Args& a) { a.d_roots_after = a.d_roots_before; }},
            {"d_roots_after=d_old_leaves+32*8", [](Args& a) { a.d_roots_after = a.d_old_leaves + 32 * 8; }},
            {"d_roots_after=d_old_leaves+32*9", [](Args& a) { a.d_roots_after = a.d_old_leaves + 32 * 9; }},
        };
        const Buf bufs[] = {{"d_leaves", &Args::d_leaves, 16},
                            {"d_offsets", &Args::d_offsets, 8},
                            {"d_levels", &Args::d_levels, 16},
                            {"d_tree_ids", &Args::d_tree_ids, 4},
                            {"d_leaf_ids", &Args::d_leaf_ids, 8},
                            {"d_new_leaves", &Args::d_new_leaves, 16},
                            {"d_order", &Args::d_order, 4},
                            {"d_old_leaves", &Args::d_old_leaves, 16},
                            {"d_siblings", &Args::d_siblings, 16},
                            {"d_positions", &Args::d_positions, 1},
                            {"d_depths", &Args::d_depths, 1},
                            {"d_roots_before", &Args::d_roots_before, 16},
                            {"d_roots_after", &Args::d_roots_after, 16},
                            {"d_roots", &Args::d_roots, 16},
                            {"d_n_bad", &Args::d_n_bad, 4},
                            {"d_n_hashed", &Args::d_n_hashed, 8}};
        null_and_misaligned(cases, bufs);
        const std::string sym = std::string(arity == 4 ? "p252_merkle4" : "p252_merkle2") + "_forest_ragged_update_sequential_device_into";
        run_cases(sym, good, cases, [arity](const Args& a) { return update(arity, a); });
    }
    delete ctx;
    return 0;
}
