// consistency_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_consistency_device_into and
// p252_merkle{4,2}_forest_consistency_verify_device_into, as a table in the format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_consistency_cpu.py compares the lines with tests/golden/consistency_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Extract {
    p252_ctx* ctx;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_old_counts, k, d_new_counts_out, d_leaves_out, d_siblings,
        d_positions, d_depths, d_n_bad;
};

int call(unsigned arity, const Extract& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_consistency_device_into : p252_merkle2_forest_ragged_consistency_device_into)(
        a.ctx, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_tree_ids), P(a.d_old_counts), a.k,
        P(a.d_new_counts_out), P(a.d_leaves_out), P(a.d_siblings), P(a.d_positions), P(a.d_depths), P(a.d_n_bad), nullptr);
}

struct Verify {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_old_counts, d_old_roots, d_new_counts, d_new_roots, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, k, d_tree_ids,
        n_trees, d_ok, d_old_roots_out, d_new_roots_out, d_n_hashed;
};

int call(unsigned arity, const Verify& a) {
    return (arity == 4 ? p252_merkle4_forest_consistency_verify_device_into : p252_merkle2_forest_consistency_verify_device_into)(
        a.ctx, a.tag, P(a.d_old_counts), P(a.d_old_roots), P(a.d_new_counts), P(a.d_new_roots), P(a.d_leaves_in), P(a.d_siblings),
        P(a.d_positions), P(a.d_depths), a.stride_depth, a.k, P(a.d_tree_ids), a.n_trees, P(a.d_ok), P(a.d_old_roots_out), P(a.d_new_roots_out),
        P(a.d_n_hashed), nullptr);
}

template <class A>
struct In {
    const char* name;
    uint64_t A::*at;
    uint64_t bytes;
};

// every output against every input and every other output: inside the other's last 16 bytes, and just behind it
template <class A, size_t NI, size_t NO>
void overlaps(std::vector<CaseOf<A>>& cases, const In<A> (&ins)[NI], const In<A> (&outs)[NO]) {
    for (size_t x = 0; x < NO; ++x) {
        const In<A> o = outs[x];
        auto add = [&](const In<A>& i) {
            const uint64_t A::*in_at = i.at;
            const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;
            cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](A& a) { a.*(o.at) = a.*in_at + last; }});
            cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](A& a) { a.*(o.at) = a.*in_at + in_bytes; }});
        };
        for (const In<A>& i : ins) add(i);
        for (size_t y = 0; y < NO; ++y)
            if (y != x) add(outs[y]);
    }
}

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        const uint64_t D = arity == 4 ? 4 : 7, per = arity - 1;  // depth(100)
        {
            const char* sym = arity == 4 ? "p252_merkle4_forest_ragged_consistency_device_into" : "p252_merkle2_forest_ragged_consistency_device_into";
            // 6 proofs out of a forest of 3 trees of at most 100 of 120 leaves
            const Extract good = {ctx, slot(0), 120, slot(1), 3, 100, slot(2), slot(3), slot(4), 6, slot(5), slot(6), slot(7), slot(8), slot(9), slot(10)};
            using Case = CaseOf<Extract>;
            using Buf = BufOf<Extract>;
            std::vector<Case> cases = {
                {"control", [](Extract&) {}},
                {"ctx=NULL", [](Extract& a) { a.ctx = nullptr; }},
                {"k=0", [](Extract& a) { a.k = 0; }},
                {"k=0,all=NULL,max_leaves=0", [ctx](Extract& a) { a = Extract{ctx, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }},
                {"max_leaves=0", [](Extract& a) { a.max_leaves = 0; }},
                {"n_trees=0", [](Extract& a) { a.n_trees = 0; }},
                {"n_leaves=0", [](Extract& a) { a.n_leaves = 0; }},
                {"max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL", [](Extract& a) { a.max_leaves = 1, a.d_levels = a.d_siblings = a.d_positions = 0; }},
                {"max_leaves=2,d_siblings=NULL", [](Extract& a) { a.max_leaves = 2, a.d_siblings = 0; }},
                {"max_leaves=2,d_positions=NULL", [](Extract& a) { a.max_leaves = 2, a.d_positions = 0; }},
                {"max_leaves=SIZE_MAX", [](Extract& a) { a.max_leaves = MAXZ; }},
                {"n_leaves=SIZE_MAX/64+1", [](Extract& a) { a.n_leaves = MAXZ / 64 + 1; }},
                {"n_trees=SIZE_MAX/8/66+1", [](Extract& a) { a.n_trees = TREES_MAX + 1; }},
                {"k=SIZE_MAX/128/D+1", [D](Extract& a) { a.k = MAXZ / 128 / D + 1; }},
                {"k=SIZE_MAX", [](Extract& a) { a.k = MAXZ; }},
            };
            const Buf bufs[] = {{"d_leaves", &Extract::d_leaves, 16},
                                {"d_offsets", &Extract::d_offsets, 8},
                                {"d_levels", &Extract::d_levels, 16},
                                {"d_tree_ids", &Extract::d_tree_ids, 4},
                                {"d_old_counts", &Extract::d_old_counts, 8},
                                {"d_new_counts_out", &Extract::d_new_counts_out, 8},
                                {"d_leaves_out", &Extract::d_leaves_out, 16},
                                {"d_siblings", &Extract::d_siblings, 16},
                                {"d_positions", &Extract::d_positions, 1},
                                {"d_depths", &Extract::d_depths, 1},
                                {"d_n_bad", &Extract::d_n_bad, 4}};
            null_and_misaligned(cases, bufs);
            const In<Extract> ins[] = {{"d_leaves", &Extract::d_leaves, 120 * 32},
                                       {"d_offsets", &Extract::d_offsets, 4 * 8},
                                       {"d_levels", &Extract::d_levels, (120 / per + 3 * D) * 32},
                                       {"d_tree_ids", &Extract::d_tree_ids, 6 * 4},
                                       {"d_old_counts", &Extract::d_old_counts, 6 * 8}};
            const In<Extract> outs[] = {{"d_new_counts_out", &Extract::d_new_counts_out, 6 * 8},
                                        {"d_leaves_out", &Extract::d_leaves_out, 6 * 32},
                                        {"d_siblings", &Extract::d_siblings, 6 * D * per * 32},
                                        {"d_positions", &Extract::d_positions, 6 * D},
                                        {"d_depths", &Extract::d_depths, 6},
                                        {"d_n_bad", &Extract::d_n_bad, 4}};
            overlaps(cases, ins, outs);
            // the siblings end inside the leaves, and where the leaves begin
            cases.push_back({"d_siblings=d_leaves-bytes+16", [D, per](Extract& a) { a.d_siblings = a.d_leaves - 6 * D * per * 32 + 16; }});
            cases.push_back({"d_siblings=d_leaves-bytes", [D, per](Extract& a) { a.d_siblings = a.d_leaves - 6 * D * per * 32; }});
            run_cases(sym, good, cases, [arity](const Extract& a) { return call(arity, a); });
        }
        {
            const char* sym = arity == 4 ? "p252_merkle4_forest_consistency_verify_device_into" : "p252_merkle2_forest_consistency_verify_device_into";
            // 6 proofs at the stride of 100 leaves, their claims named by tree id among 3 trees
            const Verify good = {ctx,     g_tag,   slot(0), slot(1), slot(2),  slot(3),  slot(4),  slot(5),  slot(6),
                                 slot(7), D,       6,       slot(8), 3,        slot(9),  slot(10), slot(11), slot(12)};
            using Case = CaseOf<Verify>;
            using Buf = BufOf<Verify>;
            std::vector<Case> cases = {
                {"control", [](Verify&) {}},
                {"ctx=NULL", [](Verify& a) { a.ctx = nullptr; }},
                {"tag=NULL", [](Verify& a) { a.tag = nullptr; }},
                {"k=0", [](Verify& a) { a.k = 0; }},
                {"k=0,all=NULL,stride_depth=65", [ctx](Verify& a) { a = Verify{ctx, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 65, 0, 0, 0, 0, 0, 0, 0}; }},
                {"stride_depth=64", [](Verify& a) { a.stride_depth = 64; }},
                {"stride_depth=65", [](Verify& a) { a.stride_depth = 65; }},
                {"stride_depth=SIZE_MAX", [](Verify& a) { a.stride_depth = MAXZ; }},
                {"stride_depth=0,d_siblings=NULL,d_positions=NULL", [](Verify& a) { a.stride_depth = 0, a.d_siblings = a.d_positions = 0; }},
                {"d_tree_ids=NULL,n_trees=0", [](Verify& a) { a.d_tree_ids = 0, a.n_trees = 0; }},
                {"n_trees=0,claims=NULL", [](Verify& a) { a.n_trees = 0, a.d_old_counts = a.d_old_roots = a.d_new_counts = a.d_new_roots = 0; }},
                {"d_tree_ids=NULL,n_trees=0,d_old_roots=NULL", [](Verify& a) { a.d_tree_ids = 0, a.n_trees = 0, a.d_old_roots = 0; }},
                {"roots_out=NULL,d_n_hashed=NULL", [](Verify& a) { a.d_old_roots_out = a.d_new_roots_out = a.d_n_hashed = 0; }},
                {"n_trees=SIZE_MAX/64+1", [](Verify& a) { a.n_trees = MAXZ / 64 + 1; }},
                {"k=SIZE_MAX/128/D+1", [D](Verify& a) { a.k = MAXZ / 128 / D + 1; }},
                {"k=SIZE_MAX", [](Verify& a) { a.k = MAXZ; }},
            };
            const Buf bufs[] = {{"d_old_counts", &Verify::d_old_counts, 8},
                                {"d_old_roots", &Verify::d_old_roots, 16},
                                {"d_new_counts", &Verify::d_new_counts, 8},
                                {"d_new_roots", &Verify::d_new_roots, 16},
                                {"d_leaves_in", &Verify::d_leaves_in, 16},
                                {"d_siblings", &Verify::d_siblings, 16},
                                {"d_positions", &Verify::d_positions, 1},
                                {"d_depths", &Verify::d_depths, 1},
                                {"d_tree_ids", &Verify::d_tree_ids, 4},
                                {"d_ok", &Verify::d_ok, 1},
                                {"d_old_roots_out", &Verify::d_old_roots_out, 16},
                                {"d_new_roots_out", &Verify::d_new_roots_out, 16},
                                {"d_n_hashed", &Verify::d_n_hashed, 8}};
            null_and_misaligned(cases, bufs);
            const In<Verify> ins[] = {{"d_old_counts", &Verify::d_old_counts, 3 * 8},
                                      {"d_old_roots", &Verify::d_old_roots, 3 * 32},
                                      {"d_new_counts", &Verify::d_new_counts, 3 * 8},
                                      {"d_new_roots", &Verify::d_new_roots, 3 * 32},
                                      {"d_leaves_in", &Verify::d_leaves_in, 6 * 32},
                                      {"d_siblings", &Verify::d_siblings, 6 * D * per * 32},
                                      {"d_positions", &Verify::d_positions, 6 * D},
                                      {"d_depths", &Verify::d_depths, 6},
                                      {"d_tree_ids", &Verify::d_tree_ids, 6 * 4}};
            const In<Verify> outs[] = {{"d_ok", &Verify::d_ok, 6},
                                       {"d_old_roots_out", &Verify::d_old_roots_out, 6 * 32},
                                       {"d_new_roots_out", &Verify::d_new_roots_out, 6 * 32},
                                       {"d_n_hashed", &Verify::d_n_hashed, 8}};
            overlaps(cases, ins, outs);
            // without tree ids the claim arrays hold k entries: the fourth claim is read, so an output on it is refused
            cases.push_back({"d_tree_ids=NULL,d_n_hashed=d_old_counts+24", [](Verify& a) { a.d_tree_ids = 0, a.d_n_hashed = a.d_old_counts + 24; }});
            cases.push_back({"d_n_hashed=d_old_counts+24", [](Verify& a) { a.d_n_hashed = a.d_old_counts + 24; }});
            run_cases(sym, good, cases, [arity](const Verify& a) { return call(arity, a); });
        }
    }
    delete ctx;
    return 0;
}
