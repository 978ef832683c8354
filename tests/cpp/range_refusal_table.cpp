// range_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_range_stride, _forest_ragged_range_proofs_device_into and
// _forest_range_verify_device_into, as a table in the format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_range_cpu.py compares the lines with tests/golden/range_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_first, d_leaf_offsets, m, k, d_leaves_out, d_proof,
        proof_stride, d_proof_lens, d_counts, d_roots, d_ok, d_roots_out, d_n_hashed, d_n_bad;
};

int extract(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_range_proofs_device_into : p252_merkle2_forest_ragged_range_proofs_device_into)(
        a.ctx, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_tree_ids), P(a.d_first),
        P(a.d_leaf_offsets), a.m, a.k, P(a.d_leaves_out), P(a.d_proof), P(a.d_proof_lens), P(a.d_counts), P(a.d_n_bad), nullptr);
}
int verify(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_range_verify_device_into : p252_merkle2_forest_range_verify_device_into)(
        a.ctx, a.tag, P(a.d_tree_ids), P(a.d_counts), P(a.d_first), P(a.d_leaf_offsets), a.m, a.max_leaves, P(a.d_leaves_out), a.k, P(a.d_proof),
        a.proof_stride, P(a.d_proof_lens), P(a.d_roots), a.n_trees, P(a.d_ok), P(a.d_roots_out), P(a.d_n_hashed), P(a.d_n_bad), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        // the stride needs no context
        const char* ssym = arity == 4 ? "p252_merkle4_forest_range_stride" : "p252_merkle2_forest_range_stride";
        auto stride = arity == 4 ? p252_merkle4_forest_range_stride : p252_merkle2_forest_range_stride;
        for (uint64_t n : {0ull, 1ull, 2ull, 4ull, 5ull, 100ull, 0xffffffffull})
            std::printf("%s\tmax_leaves=%llu\t%llu\t\n", ssym, (unsigned long long)n, (unsigned long long)stride(n));
        // 4 runs of 9 leaves in all out of 3 trees of at most 100 of 120 leaves; the proof rows at the stride of 100 leaves
        const Args good = {ctx,     g_tag,   slot(0), 120,     slot(1), 3,        100,      slot(2),  slot(3),  slot(4),  slot(5), 4,
                           9,       slot(6), slot(7), stride(100), slot(8), slot(9), slot(10), slot(11), slot(12), slot(13), slot(14)};
        std::vector<Case> shape = {
            {"control", [](Args&) {}},
            {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
            {"m=0", [](Args& a) { a.m = 0; }},
            {"k=0", [](Args& a) { a.k = 0; }},
            {"n_trees=0", [](Args& a) { a.n_trees = 0; }},
            {"max_leaves=0", [](Args& a) { a.max_leaves = 0; }},
            {"k+2m=2^32-1", [](Args& a) { a.k = 0xffffffffull - 8; }},
            {"k+2m=2^32", [](Args& a) { a.k = 0xffffffffull - 7; }},
            {"k=2^32-1", [](Args& a) { a.k = 0xffffffffull; }},
            {"k=2^32", [](Args& a) { a.k = 1ull << 32; }},
            {"k=SIZE_MAX", [](Args& a) { a.k = MAXZ; }},
            {"m=2^31-5,k+2m=2^32-1", [](Args& a) { a.m = 0x7ffffffbull; }},
            {"m=2^31", [](Args& a) { a.m = 0x80000000ull; }},
            {"m=2^32", [](Args& a) { a.m = 1ull << 32; }},
            {"m=SIZE_MAX", [](Args& a) { a.m = MAXZ; }},
            {"max_leaves=2^32-1", [](Args& a) { a.max_leaves = 0xffffffffull; }},
            {"max_leaves=2^32", [](Args& a) { a.max_leaves = 1ull << 32; }},
            {"max_leaves=SIZE_MAX", [](Args& a) { a.max_leaves = MAXZ; }},
            {"counters=NULL", [](Args& a) { a.d_n_bad = a.d_n_hashed = a.d_roots_out = 0; }},
        };
        const std::vector<Case> eshape = {
            {"n_leaves=0", [](Args& a) { a.n_leaves = 0; }},
            {"max_leaves=1,d_levels=NULL,d_proof=NULL", [](Args& a) { a.max_leaves = 1, a.d_levels = a.d_proof = 0; }},
            {"max_leaves=2,d_levels=NULL", [](Args& a) { a.max_leaves = 2, a.d_levels = 0; }},
            {"max_leaves=2,d_proof=NULL", [](Args& a) { a.max_leaves = 2, a.d_proof = 0; }},
            {"n_leaves=SIZE_MAX/64+1", [](Args& a) { a.n_leaves = MAXZ / 64 + 1; }},
            {"n_trees=SIZE_MAX/8/66+1", [](Args& a) { a.n_trees = TREES_MAX + 1; }},
            {"n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2",
             [](Args& a) { a.n_leaves = 1ull << 40, a.max_leaves = 1ull << 31, a.n_trees = ((MAXZ / 2) >> 31) + 1; }},
        };
        const std::vector<Case> vshape = {
            {"tag=NULL", [](Args& a) { a.tag = nullptr; }},
            {"proof_stride=0,d_proof=NULL", [](Args& a) { a.proof_stride = 0, a.d_proof = 0; }},
            {"proof_stride=1000", [](Args& a) { a.proof_stride = 1000; }},
            {"m*proof_stride=SIZE_MAX>>8", [](Args& a) { a.proof_stride = (MAXZ >> 8) / 4; }},
            {"m*proof_stride>SIZE_MAX>>8", [](Args& a) { a.proof_stride = (MAXZ >> 8) / 4 + 1; }},
            {"proof_stride=SIZE_MAX", [](Args& a) { a.proof_stride = MAXZ; }},
            {"n_trees=SIZE_MAX/32", [](Args& a) { a.n_trees = MAXZ / 32; }},
            {"n_trees=SIZE_MAX/32+1", [](Args& a) { a.n_trees = MAXZ / 32 + 1; }},
        };
        const Buf ebufs[] = {{"d_leaves", &Args::d_leaves, 16},       {"d_offsets", &Args::d_offsets, 8},       {"d_levels", &Args::d_levels, 16},
                             {"d_tree_ids", &Args::d_tree_ids, 4},    {"d_first", &Args::d_first, 8},           {"d_leaf_offsets", &Args::d_leaf_offsets, 8},
                             {"d_leaves_out", &Args::d_leaves_out, 16}, {"d_proof", &Args::d_proof, 16},        {"d_proof_lens", &Args::d_proof_lens, 4},
                             {"d_counts_out", &Args::d_counts, 8},    {"d_n_bad", &Args::d_n_bad, 4}};
        const Buf vbufs[] = {{"d_tree_ids", &Args::d_tree_ids, 4},    {"d_counts", &Args::d_counts, 8},         {"d_first", &Args::d_first, 8},
                             {"d_leaf_offsets", &Args::d_leaf_offsets, 8}, {"d_leaves_in", &Args::d_leaves_out, 16}, {"d_proof", &Args::d_proof, 16},
                             {"d_proof_lens", &Args::d_proof_lens, 4}, {"d_roots", &Args::d_roots, 16},         {"d_ok", &Args::d_ok, 1},
                             {"d_roots_out", &Args::d_roots_out, 16}, {"d_n_hashed", &Args::d_n_hashed, 8},     {"d_n_bad", &Args::d_n_bad, 4}};
        for (int which = 0; which < 2; ++which) {
            const std::string sym = std::string(arity == 4 ? "p252_merkle4" : "p252_merkle2") +
                                    (which ? "_forest_range_verify_device_into" : "_forest_ragged_range_proofs_device_into");
            std::vector<Case> cases = shape;
            for (const Case& c : which ? vshape : eshape) cases.push_back(c);
            which ? null_and_misaligned(cases, vbufs) : null_and_misaligned(cases, ebufs);
            run_cases(sym, good, cases, [arity, which](const Args& a) { return which ? verify(arity, a) : extract(arity, a); });
        }
    }
    delete ctx;
    return 0;
}
