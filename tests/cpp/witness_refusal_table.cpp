// witness_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_frontier_append_witness_device_into as a table in the
// format of api_refusals.cpp:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_witness_cpu.py compares the lines with tests/golden/witness_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Append {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, n_add, d_add_offsets;
    uint64_t d_wit_tree_ids, d_wit_leaf_ids, k, d_wit_leaves, d_wit_siblings, d_wit_positions, d_wit_depths;
    uint64_t d_n_bad, d_n_hashed, d_n_bad_witness;
};

int call(unsigned arity, const Append& a) {
    return (arity == 4 ? p252_merkle4_forest_frontier_append_witness_device_into : p252_merkle2_forest_frontier_append_witness_device_into)(
        a.ctx, a.tag, P(a.d_counts), P(a.d_frontier), P(a.d_roots), a.n_trees, a.max_leaves, P(a.d_add), a.n_add, P(a.d_add_offsets),
        P(a.d_wit_tree_ids), P(a.d_wit_leaf_ids), a.k, P(a.d_wit_leaves), P(a.d_wit_siblings), P(a.d_wit_positions), P(a.d_wit_depths),
        P(a.d_n_bad), P(a.d_n_hashed), P(a.d_n_bad_witness), nullptr);
}

struct Range {
    const char* name;
    uint64_t Append::*at;
    uint64_t bytes;
};

// the witness buffers far from everything and from each other: for the rows whose k makes them large
void spread(Append& a) {
    a.d_wit_tree_ids = 1ull << 56, a.d_wit_leaf_ids = 2ull << 56, a.d_wit_leaves = 3ull << 56, a.d_wit_siblings = 4ull << 56;
    a.d_wit_positions = 5ull << 56, a.d_wit_depths = 6ull << 56;
}

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        const char* sym =
            arity == 4 ? "p252_merkle4_forest_frontier_append_witness_device_into" : "p252_merkle2_forest_frontier_append_witness_device_into";
        // 5 trees of at most 100 leaves (depth D = 4 / 7: 15 / 8 scalars of frontier each) receive 12 leaves under 6 witnesses
        const uint64_t stride = arity == 4 ? 15 : 8, D = arity == 4 ? 4 : 7, k = 6;
        const Append good = {ctx,     g_tag,   slot(0), slot(1), slot(2),  5,        100,      slot(3),  12,       slot(4),
                             slot(5), slot(6), k,       slot(7), slot(8),  slot(9),  slot(10), slot(11), slot(12), slot(13)};
        using Case = CaseOf<Append>;
        using Buf = BufOf<Append>;
        std::vector<Case> cases = {
            {"control", [](Append&) {}},
            {"ctx=NULL", [](Append& a) { a.ctx = nullptr; }},
            {"tag=NULL", [](Append& a) { a.tag = nullptr; }},
            // the plain call's own rows
            {"n_trees=0,k=0", [](Append& a) { a.n_trees = a.k = 0; }},
            {"n_trees=0,k=0,max_leaves=0", [](Append& a) { a.n_trees = a.k = a.max_leaves = 0; }},
            {"n_trees=0", [](Append& a) { a.n_trees = 0; }},  // (every witness is a bad one: the call goes on to the device)
            {"n_trees=0,state=NULL", [](Append& a) { a.n_trees = 0, a.d_counts = a.d_frontier = a.d_roots = a.d_add_offsets = 0; }},
            {"n_trees=0,max_leaves=0", [](Append& a) { a.n_trees = a.max_leaves = 0; }},
            {"max_leaves=0", [](Append& a) { a.max_leaves = 0; }},
            {"max_leaves=1", [](Append& a) { a.max_leaves = 1; }},
            {"max_leaves=1,d_wit_siblings=NULL,d_wit_positions=NULL", [](Append& a) { a.max_leaves = 1, a.d_wit_siblings = a.d_wit_positions = 0; }},
            {"max_leaves=2,d_wit_siblings=NULL", [](Append& a) { a.max_leaves = 2, a.d_wit_siblings = 0; }},
            {"max_leaves=2,d_wit_positions=NULL", [](Append& a) { a.max_leaves = 2, a.d_wit_positions = 0; }},
            {"max_leaves=SIZE_MAX", [](Append& a) { a.max_leaves = MAXZ; }},
            {"n_add=0", [](Append& a) { a.n_add = 0; }},
            {"n_add=0,d_add=NULL", [](Append& a) { a.n_add = 0, a.d_add = 0; }},
            {"n_add=2^32-1", [](Append& a) { a.n_add = 0xffffffffull, a.d_add = 1ull << 50; }},
            {"n_add=2^32", [](Append& a) { a.n_add = 1ull << 32; }},
            {"n_add=SIZE_MAX", [](Append& a) { a.n_add = MAXZ; }},
            {"n_trees=SIZE_MAX/8/66+1", [](Append& a) { a.n_trees = TREES_MAX + 1; }},
            {"n_trees=SIZE_MAX/64/bound+1", [stride](Append& a) { a.n_trees = MAXZ / 64 / stride + 1; }},
            {"n_trees*n_add>SIZE_MAX/2", [](Append& a) { a.n_add = 1ull << 31, a.n_trees = ((MAXZ / 2) >> 31) + 1, a.max_leaves = 1; }},
            // k == 0 is the plain call: the witness buffers are not looked at
            {"k=0", [](Append& a) { a.k = 0; }},
            {"k=0,witness=NULL",
             [](Append& a) {
                 a.k = 0;
                 a.d_wit_tree_ids = a.d_wit_leaf_ids = a.d_wit_leaves = a.d_wit_siblings = a.d_wit_positions = a.d_wit_depths = a.d_n_bad_witness = 0;
             }},
            {"k=0,d_wit_leaves+8", [](Append& a) { a.k = 0, a.d_wit_leaves += 8; }},
            {"k=0,d_wit_leaves=d_add", [](Append& a) { a.k = 0, a.d_wit_leaves = a.d_add; }},
            // the sizes: k D (A - 1) 32 bytes of siblings inside size_t, floor(256 / D) witnesses per block inside a grid
            {"k=SIZE_MAX/128/D", [D](Append& a) { a.k = MAXZ / 128 / D, spread(a); }},
            {"k=SIZE_MAX/128/D+1", [D](Append& a) { a.k = MAXZ / 128 / D + 1, spread(a); }},
            {"k=SIZE_MAX", [](Append& a) { a.k = MAXZ, spread(a); }},
            {"k=(256/D)*(2^31-1)", [D](Append& a) { a.k = (256 / D) * 0x7fffffffull, spread(a); }},
            {"k=(256/D)*(2^31-1)+1", [D](Append& a) { a.k = (256 / D) * 0x7fffffffull + 1, spread(a); }},
            {"max_leaves=1,k=256*(2^31-1)", [](Append& a) { a.max_leaves = 1, a.k = 256 * 0x7fffffffull, spread(a); }},
            {"max_leaves=1,k=256*(2^31-1)+1", [](Append& a) { a.max_leaves = 1, a.k = 256 * 0x7fffffffull + 1, spread(a); }},
        };
        const Buf bufs[] = {{"d_counts", &Append::d_counts, 8},
                            {"d_frontier", &Append::d_frontier, 16},
                            {"d_roots", &Append::d_roots, 16},
                            {"d_add", &Append::d_add, 16},
                            {"d_add_offsets", &Append::d_add_offsets, 8},
                            {"d_wit_tree_ids", &Append::d_wit_tree_ids, 4},
                            {"d_wit_leaf_ids", &Append::d_wit_leaf_ids, 8},
                            {"d_wit_leaves", &Append::d_wit_leaves, 16},
                            {"d_wit_siblings", &Append::d_wit_siblings, 16},
                            {"d_wit_positions", &Append::d_wit_positions, 1},
                            {"d_wit_depths", &Append::d_wit_depths, 1},
                            {"d_n_bad", &Append::d_n_bad, 4},
                            {"d_n_hashed", &Append::d_n_hashed, 8},
                            {"d_n_bad_witness", &Append::d_n_bad_witness, 4}};
        null_and_misaligned(cases, bufs);
        // the plain call's overlaps: the state and the counters against the two inputs
        const Range ins[] = {{"d_add", &Append::d_add, 12 * 32}, {"d_add_offsets", &Append::d_add_offsets, 6 * 8}};
        const Range state[] = {{"d_counts", &Append::d_counts, 5 * 8},
                               {"d_frontier", &Append::d_frontier, 5 * stride * 32},
                               {"d_roots", &Append::d_roots, 5 * 32},
                               {"d_n_bad", &Append::d_n_bad, 4},
                               {"d_n_hashed", &Append::d_n_hashed, 8}};
        auto pair = [&cases](const Range& o, const Range& i) {
            uint64_t Append::*o_at = o.at;
            uint64_t Append::*i_at = i.at;
            const uint64_t last = (i.bytes - 1) & ~15ull, end = (i.bytes + 15) & ~15ull;  // inside the last 16 bytes, and just behind it
            cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o_at, i_at, last](Append& a) { a.*o_at = a.*i_at + last; }});
            cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o_at, i_at, end](Append& a) { a.*o_at = a.*i_at + end; }});
        };
        for (const Range& o : state)
            for (const Range& i : ins) pair(o, i);
        // what the witnesses' pass writes against everything else the call names, and against each other
        const Range ids[] = {{"d_wit_tree_ids", &Append::d_wit_tree_ids, k * 4}, {"d_wit_leaf_ids", &Append::d_wit_leaf_ids, k * 8}};
        const Range mine[] = {{"d_wit_leaves", &Append::d_wit_leaves, k * 32},
                              {"d_wit_siblings", &Append::d_wit_siblings, k * D * (arity - 1) * 32},
                              {"d_wit_positions", &Append::d_wit_positions, k * D},
                              {"d_wit_depths", &Append::d_wit_depths, k},
                              {"d_n_bad_witness", &Append::d_n_bad_witness, 4}};
        for (const Range& o : mine) {
            for (const Range& i : state) pair(o, i);
            for (const Range& i : ins) pair(o, i);
            for (const Range& i : ids) pair(o, i);
            for (const Range& i : mine)
                if (i.at != o.at) pair(o, i);
        }
        // a witness array that ends inside d_add, and where d_add begins
        cases.push_back({"d_wit_siblings=d_add-bytes+16", [=](Append& a) { a.d_wit_siblings = a.d_add - k * D * (arity - 1) * 32 + 16; }});
        cases.push_back({"d_wit_siblings=d_add-bytes", [=](Append& a) { a.d_wit_siblings = a.d_add - k * D * (arity - 1) * 32; }});
        run_cases(sym, good, cases, [arity](const Append& a) { return call(arity, a); });
    }
    delete ctx;
    return 0;
}
