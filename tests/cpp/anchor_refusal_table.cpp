// anchor_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_anchor_openings_device_into, as a table in the
// format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_anchor_cpu.py compares the lines with tests/golden/anchor_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Anchor {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_anchor_tree_ids, d_anchor_counts, m, d_anchor_ids, d_leaf_ids, k,
        d_anchor_roots, d_anchor_depths, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad_anchors, d_n_bad, d_n_hashed;
};

int call(unsigned arity, const Anchor& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_anchor_openings_device_into : p252_merkle2_forest_ragged_anchor_openings_device_into)(
        a.ctx, a.tag, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_anchor_tree_ids),
        P(a.d_anchor_counts), a.m, P(a.d_anchor_ids), P(a.d_leaf_ids), a.k, P(a.d_anchor_roots), P(a.d_anchor_depths), P(a.d_leaves_out),
        P(a.d_siblings), P(a.d_positions), P(a.d_depths), P(a.d_n_bad_anchors), P(a.d_n_bad), P(a.d_n_hashed), nullptr);
}

struct In {
    const char* name;
    uint64_t Anchor::*at;
    uint64_t bytes;
};

// every output against every input and every other output: inside the other's last 16 bytes, and just behind it
template <size_t NI, size_t NO>
void overlaps(std::vector<CaseOf<Anchor>>& cases, const In (&ins)[NI], const In (&outs)[NO]) {
    for (size_t x = 0; x < NO; ++x) {
        const In o = outs[x];
        auto add = [&](const In& i) {
            uint64_t Anchor::*const in_at = i.at;
            const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;
            cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Anchor& a) { a.*(o.at) = a.*in_at + last; }});
            cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Anchor& a) { a.*(o.at) = a.*in_at + in_bytes; }});
        };
        for (const In& i : ins) add(i);
        for (size_t y = 0; y < NO; ++y)
            if (y != x) add(outs[y]);
    }
}

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        const uint64_t D = arity == 4 ? 4 : 7, per = arity - 1;  // depth(100)
        const char* sym = arity == 4 ? "p252_merkle4_forest_ragged_anchor_openings_device_into" : "p252_merkle2_forest_ragged_anchor_openings_device_into";
        // 5 anchors and 6 openings out of a forest of 3 trees of at most 100 of 120 leaves
        const Anchor good = {ctx,     g_tag,   slot(0), 120,      slot(1),  3,        100,      slot(2),  slot(3),  slot(4),  5,       slot(5),
                             slot(6), 6,       slot(7), slot(8),  slot(9),  slot(10), slot(11), slot(12), slot(13), slot(14), slot(15)};
        using Case = CaseOf<Anchor>;
        using Buf = BufOf<Anchor>;
        std::vector<Case> cases = {
            {"control", [](Anchor&) {}},
            {"ctx=NULL", [](Anchor& a) { a.ctx = nullptr; }},
            {"tag=NULL", [](Anchor& a) { a.tag = nullptr; }},
            {"m=0,k=0", [](Anchor& a) { a.m = a.k = 0; }},
            {"m=0,k=0,all=NULL,max_leaves=0", [ctx](Anchor& a) { a = Anchor{ctx, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }},
            // the roots alone: nothing of the openings is looked at
            {"k=0", [](Anchor& a) { a.k = 0; }},
            {"k=0,openings=NULL", [](Anchor& a) { a.k = 0, a.d_anchor_ids = a.d_leaf_ids = a.d_leaves_out = a.d_siblings = a.d_positions = a.d_depths = 0; }},
            {"k=0,d_anchor_roots=NULL", [](Anchor& a) { a.k = 0, a.d_anchor_roots = 0; }},
            // no anchor: every opening is bad, nothing of the anchors is looked at
            {"m=0", [](Anchor& a) { a.m = 0; }},
            {"m=0,anchors=NULL", [](Anchor& a) { a.m = 0, a.d_anchor_tree_ids = a.d_anchor_counts = a.d_anchor_roots = a.d_anchor_depths = 0; }},
            {"m=0,d_leaves_out=NULL", [](Anchor& a) { a.m = 0, a.d_leaves_out = 0; }},
            {"max_leaves=0", [](Anchor& a) { a.max_leaves = 0; }},
            {"n_trees=0", [](Anchor& a) { a.n_trees = 0; }},
            {"n_leaves=0", [](Anchor& a) { a.n_leaves = 0; }},
            {"max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL", [](Anchor& a) { a.max_leaves = 1, a.d_levels = a.d_siblings = a.d_positions = 0; }},
            {"max_leaves=2,d_levels=NULL", [](Anchor& a) { a.max_leaves = 2, a.d_levels = 0; }},
            {"max_leaves=2,d_siblings=NULL", [](Anchor& a) { a.max_leaves = 2, a.d_siblings = 0; }},
            {"max_leaves=2,d_positions=NULL", [](Anchor& a) { a.max_leaves = 2, a.d_positions = 0; }},
            {"max_leaves=SIZE_MAX", [](Anchor& a) { a.max_leaves = MAXZ; }},
            {"counters=NULL", [](Anchor& a) { a.d_n_bad_anchors = a.d_n_bad = a.d_n_hashed = 0; }},
            {"n_leaves=SIZE_MAX/64+1", [](Anchor& a) { a.n_leaves = MAXZ / 64 + 1; }},
            {"n_trees=SIZE_MAX/8/66+1", [](Anchor& a) { a.n_trees = TREES_MAX + 1; }},
            {"m=2^32-1", [](Anchor& a) { a.m = 0xffffffffull; }},
            {"m=2^32", [](Anchor& a) { a.m = 1ull << 32; }},
            {"m=SIZE_MAX", [](Anchor& a) { a.m = MAXZ; }},
            {"k=SIZE_MAX/128/D+1", [D](Anchor& a) { a.k = MAXZ / 128 / D + 1; }},
            {"k=SIZE_MAX", [](Anchor& a) { a.k = MAXZ; }},
        };
        const Buf bufs[] = {{"d_leaves", &Anchor::d_leaves, 16},
                            {"d_offsets", &Anchor::d_offsets, 8},
                            {"d_levels", &Anchor::d_levels, 16},
                            {"d_anchor_tree_ids", &Anchor::d_anchor_tree_ids, 4},
                            {"d_anchor_counts", &Anchor::d_anchor_counts, 8},
                            {"d_anchor_ids", &Anchor::d_anchor_ids, 4},
                            {"d_leaf_ids", &Anchor::d_leaf_ids, 8},
                            {"d_anchor_roots", &Anchor::d_anchor_roots, 16},
                            {"d_anchor_depths", &Anchor::d_anchor_depths, 1},
                            {"d_leaves_out", &Anchor::d_leaves_out, 16},
                            {"d_siblings", &Anchor::d_siblings, 16},
                            {"d_positions", &Anchor::d_positions, 1},
                            {"d_depths", &Anchor::d_depths, 1},
                            {"d_n_bad_anchors", &Anchor::d_n_bad_anchors, 4},
                            {"d_n_bad", &Anchor::d_n_bad, 4},
                            {"d_n_hashed", &Anchor::d_n_hashed, 8}};
        null_and_misaligned(cases, bufs);
        const In ins[] = {{"d_leaves", &Anchor::d_leaves, 120 * 32},
                          {"d_offsets", &Anchor::d_offsets, 4 * 8},
                          {"d_levels", &Anchor::d_levels, (120 / per + 3 * D) * 32},
                          {"d_anchor_tree_ids", &Anchor::d_anchor_tree_ids, 5 * 4},
                          {"d_anchor_counts", &Anchor::d_anchor_counts, 5 * 8},
                          {"d_anchor_ids", &Anchor::d_anchor_ids, 6 * 4},
                          {"d_leaf_ids", &Anchor::d_leaf_ids, 6 * 8}};
        const In outs[] = {{"d_anchor_roots", &Anchor::d_anchor_roots, 5 * 32},
                           {"d_anchor_depths", &Anchor::d_anchor_depths, 5},
                           {"d_leaves_out", &Anchor::d_leaves_out, 6 * 32},
                           {"d_siblings", &Anchor::d_siblings, 6 * D * per * 32},
                           {"d_positions", &Anchor::d_positions, 6 * D},
                           {"d_depths", &Anchor::d_depths, 6},
                           {"d_n_bad_anchors", &Anchor::d_n_bad_anchors, 4},
                           {"d_n_bad", &Anchor::d_n_bad, 4},
                           {"d_n_hashed", &Anchor::d_n_hashed, 8}};
        overlaps(cases, ins, outs);
        // the siblings end inside the leaves, and where the leaves begin
        cases.push_back({"d_siblings=d_leaves-bytes+16", [D, per](Anchor& a) { a.d_siblings = a.d_leaves - 6 * D * per * 32 + 16; }});
        cases.push_back({"d_siblings=d_leaves-bytes", [D, per](Anchor& a) { a.d_siblings = a.d_leaves - 6 * D * per * 32; }});
        // with no opening the opening arrays have no bytes: one of them on an input is no overlap
        cases.push_back({"k=0,d_leaves_out=d_leaves", [](Anchor& a) { a.k = 0, a.d_leaves_out = a.d_leaves; }});
        run_cases(sym, good, cases, [arity](const Anchor& a) { return call(arity, a); });
    }
    delete ctx;
    return 0;
}
