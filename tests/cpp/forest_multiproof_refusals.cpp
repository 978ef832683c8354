// forest_multiproof_refusals.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_multiproof_bound / _device / _verify_device,
// as a table, in the format of api_refusals.cpp:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_multiproof_cpu.py compares the lines with tests/golden/forest_multiproof_refusals.txt; api_refusals.cpp
// tables the entry points whose names end in `_device`, these — `_device_into`, as the append's — have their table here.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k, d_leaves_out, d_proof, proof_len, d_proof_offsets,
        d_roots, d_ok, d_roots_out, d_n_hashed, d_n_bad;
};

int extract(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_multiproof_device_into : p252_merkle2_forest_ragged_multiproof_device_into)(
        a.ctx, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_tree_ids), P(a.d_leaf_ids), a.k,
        P(a.d_leaves_out), P(a.d_proof), a.proof_len, P(a.d_proof_offsets), P(a.d_n_bad), nullptr);
}
int verify(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_multiproof_verify_device_into : p252_merkle2_forest_ragged_multiproof_verify_device_into)(
        a.ctx, a.tag, P(a.d_offsets), a.n_leaves, a.n_trees, a.max_leaves, P(a.d_tree_ids), P(a.d_leaf_ids), P(a.d_leaves_out), a.k, P(a.d_proof),
        a.proof_len, P(a.d_proof_offsets), P(a.d_roots), P(a.d_ok), P(a.d_roots_out), P(a.d_n_hashed), P(a.d_n_bad), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        // the bound needs no context: its zero rows and one value
        const char* bsym = arity == 4 ? "p252_merkle4_forest_ragged_multiproof_bound" : "p252_merkle2_forest_ragged_multiproof_bound";
        auto bound = arity == 4 ? p252_merkle4_forest_ragged_multiproof_bound : p252_merkle2_forest_ragged_multiproof_bound;
        const struct {
            const char* name;
            uint64_t n_leaves, n_trees, max_leaves, k;
        } brows[] = {{"control", 12, 3, 5, 4}, {"k=0", 12, 3, 5, 0}, {"n_leaves=0", 0, 3, 5, 4}, {"n_trees=0", 12, 0, 5, 4},
                     {"max_leaves=1", 12, 3, 1, 4}, {"k=1000", 12, 3, 5, 1000}};
        for (const auto& b : brows)
            std::printf("%s\t%s\t%llu\t\n", bsym, b.name, (unsigned long long)bound(b.n_leaves, b.n_trees, b.max_leaves, b.k));
        // 3 trees of at most 5 of 12 leaves, 4 pairs, a proof of 7 scalars
        const Args good = {ctx,     g_tag,   slot(0), 12, slot(1),  3,        5,        slot(2),  slot(3),  slot(4),
                           4,       slot(5), slot(6), 7,  slot(7),  slot(8),  slot(9),  slot(10), slot(11), slot(12)};
        std::vector<Case> shape = {
            {"control", [](Args&) {}},
            {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
            {"k=0", [](Args& a) { a.k = 0; }},
            {"n_trees=0", [](Args& a) { a.n_trees = 0; }},
            {"n_leaves=0", [](Args& a) { a.n_leaves = 0; }},
            {"max_leaves=0", [](Args& a) { a.max_leaves = 0; }},
            {"k=2^32-1", [](Args& a) { a.k = 0xffffffffull; }},
            {"k=2^32", [](Args& a) { a.k = 1ull << 32; }},
            {"max_leaves=2^32-1", [](Args& a) { a.max_leaves = 0xffffffffull; }},
            {"max_leaves=2^32", [](Args& a) { a.max_leaves = 1ull << 32; }},
            {"max_leaves=1,d_levels=NULL", [](Args& a) { a.max_leaves = 1, a.d_levels = 0; }},
            {"proof_len=0,d_proof=NULL", [](Args& a) { a.proof_len = 0, a.d_proof = 0; }},
            {"proof_len=SIZE_MAX/32", [](Args& a) { a.proof_len = MAXZ / 32; }},
            {"proof_len=SIZE_MAX/32+1", [](Args& a) { a.proof_len = MAXZ / 32 + 1; }},
            {"n_leaves=SIZE_MAX/64+1", [](Args& a) { a.n_leaves = MAXZ / 64 + 1; }},
            {"n_trees=SIZE_MAX/8/66+1", [](Args& a) { a.n_trees = MAXZ / 8 / 66 + 1; }},
            {"n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2",
             [](Args& a) { a.n_leaves = 1ull << 40, a.max_leaves = 1ull << 31, a.n_trees = ((MAXZ / 2) >> 31) + 1; }},
        };
        const Buf ebufs[] = {{"d_leaves", &Args::d_leaves, 16},         {"d_offsets", &Args::d_offsets, 8},   {"d_levels", &Args::d_levels, 16},
                             {"d_tree_ids", &Args::d_tree_ids, 4},      {"d_leaf_ids", &Args::d_leaf_ids, 8}, {"d_leaves_out", &Args::d_leaves_out, 16},
                             {"d_proof", &Args::d_proof, 16},           {"d_proof_offsets", &Args::d_proof_offsets, 8},
                             {"d_n_bad", &Args::d_n_bad, 4}};
        const Buf vbufs[] = {{"d_offsets", &Args::d_offsets, 8},       {"d_tree_ids", &Args::d_tree_ids, 4}, {"d_leaf_ids", &Args::d_leaf_ids, 8},
                             {"d_leaves_in", &Args::d_leaves_out, 16}, {"d_proof", &Args::d_proof, 16},      {"d_proof_offsets", &Args::d_proof_offsets, 8},
                             {"d_roots", &Args::d_roots, 16},          {"d_ok", &Args::d_ok, 1},             {"d_roots_out", &Args::d_roots_out, 16},
                             {"d_n_hashed", &Args::d_n_hashed, 8},     {"d_n_bad", &Args::d_n_bad, 4}};
        for (int which = 0; which < 2; ++which) {
            const std::string sym = std::string(arity == 4 ? "p252_merkle4" : "p252_merkle2") +
                                    (which ? "_forest_ragged_multiproof_verify_device_into" : "_forest_ragged_multiproof_device_into");
            std::vector<Case> cases = shape;
            if (which) cases.push_back({"tag=NULL", [](Args& a) { a.tag = nullptr; }});
            // every buffer NULL, and off its alignment
            which ? null_and_misaligned(cases, vbufs) : null_and_misaligned(cases, ebufs);
            run_cases(sym, good, cases, [arity, which](const Args& a) { return which ? verify(arity, a) : extract(arity, a); });
        }
    }
    delete ctx;
    return 0;
}
