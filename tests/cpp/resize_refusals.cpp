// resize_refusals.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_resize_device_into, as a table, in the format of
// api_refusals.cpp and append_refusals.cpp (whose cases these are, plus d_keep and fewer trees):
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_resize_cpu.py compares the lines with tests/golden/resize_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, n_add, d_add_offsets, n_trees_new, max_leaves_new, d_leaves_new,
        leaves_cap, d_offsets_new, d_levels_new, levels_cap, d_roots, d_n_bad, d_n_hashed;
};

int call(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_resize_device_into : p252_merkle2_forest_ragged_resize_device_into)(
        a.ctx, a.tag, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves, P(a.d_levels), P(a.d_keep), P(a.d_add), a.n_add, P(a.d_add_offsets),
        a.n_trees_new, a.max_leaves_new, P(a.d_leaves_new), a.leaves_cap, P(a.d_offsets_new), P(a.d_levels_new), a.levels_cap, P(a.d_roots),
        P(a.d_n_bad), P(a.d_n_hashed), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        const char* sym = arity == 4 ? "p252_merkle4_forest_ragged_resize_device_into" : "p252_merkle2_forest_ragged_resize_device_into";
        // 3 old trees of at most 5 of 12 leaves; 4 new trees of at most 9 of 12 + 6 leaves
        const uint64_t depth_new = arity == 4 ? 2 : 4, need = 18 / (arity - 1) + 4 * depth_new;
        const Args good = {ctx, g_tag, slot(0), 12, slot(1), 3, 5, slot(2), slot(11), slot(3), 6, slot(4), 4, 9, slot(5), 18, slot(6), slot(7), need, slot(8),
                           slot(9), slot(10)};
        std::vector<Case> cases = {
            {"control", [](Args&) {}},
            {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
            {"tag=NULL", [](Args& a) { a.tag = nullptr; }},
            // the sizes
            {"n_trees_new=0", [](Args& a) { a.n_trees_new = 0; }},
            {"n_trees_new=0,max_leaves_new=0", [](Args& a) { a.n_trees_new = a.max_leaves_new = 0; }},
            {"n_trees_new=n_trees-1", [](Args& a) { a.n_trees_new = 2; }},
            {"n_trees_new=n_trees", [](Args& a) { a.n_trees_new = 3; }},
            {"n_trees_new=1", [](Args& a) { a.n_trees_new = 1; }},
            {"d_keep=NULL,n_trees_new=n_trees-1", [](Args& a) { a.d_keep = 0, a.n_trees_new = 2; }},
            {"n_add=0,d_add=NULL,d_keep=NULL", [](Args& a) { a.n_add = 0, a.d_add = a.d_keep = 0; }},
            {"max_leaves_new=max_leaves-1", [](Args& a) { a.max_leaves_new = 4; }},
            {"max_leaves_new=max_leaves", [](Args& a) { a.max_leaves_new = 5; }},
            {"max_leaves_new=0,max_leaves=0,n_trees=0", [](Args& a) { a.max_leaves_new = a.max_leaves = a.n_trees = 0; }},
            {"max_leaves=0", [](Args& a) { a.max_leaves = 0; }},
            {"leaves_cap=n_leaves+n_add-1", [](Args& a) { a.leaves_cap = 17; }},
            {"leaves_cap=n_leaves+n_add+7", [](Args& a) { a.leaves_cap = 25; }},
            {"levels_cap=need-1", [need](Args& a) { a.levels_cap = need - 1; }},
            {"levels_cap=need+1", [need](Args& a) { a.levels_cap = need + 1; }},
            {"levels_cap=0", [](Args& a) { a.levels_cap = 0; }},
            {"n_add=0,d_add=NULL", [](Args& a) { a.n_add = 0, a.d_add = 0; }},
            {"n_trees=0,d_leaves=d_offsets=d_levels=NULL,n_leaves=0", [](Args& a) { a.n_trees = a.n_leaves = a.d_leaves = a.d_offsets = a.d_levels = 0; }},
            {"max_leaves=1,d_levels=NULL", [](Args& a) { a.max_leaves = 1, a.d_levels = 0; }},
            {"max_leaves=max_leaves_new=1,d_levels=d_levels_new=NULL", [](Args& a) { a.max_leaves = a.max_leaves_new = 1, a.d_levels = a.d_levels_new = 0; }},
            {"max_leaves=1,max_leaves_new=2,d_levels=d_levels_new=NULL", [](Args& a) { a.max_leaves = 1, a.max_leaves_new = 2, a.d_levels = a.d_levels_new = 0; }},
            // overflow
            {"n_leaves=SIZE_MAX/64+1", [](Args& a) { a.n_leaves = MAXZ / 64 + 1; }},
            {"n_add=SIZE_MAX/64+1", [](Args& a) { a.n_add = MAXZ / 64 + 1; }},
            {"n_add=SIZE_MAX", [](Args& a) { a.n_add = MAXZ; }},
            {"leaves_cap=SIZE_MAX/64+1", [](Args& a) { a.leaves_cap = MAXZ / 64 + 1; }},
            {"levels_cap=SIZE_MAX/64+1", [](Args& a) { a.levels_cap = MAXZ / 64 + 1; }},
            {"n_trees_new=SIZE_MAX/8/66+1", [](Args& a) { a.n_trees_new = MAXZ / 8 / 66 + 1; }},
            {"n_trees_new*min(max_leaves_new,n_leaves+n_add)>SIZE_MAX/2",
             [](Args& a) { a.n_add = 1ull << 40, a.max_leaves_new = 1ull << 41, a.n_trees_new = ((MAXZ / 2) >> 40) + 1; }},
        };
        // every buffer NULL, and off its alignment
        const Buf bufs[] = {{"d_leaves", &Args::d_leaves, 16},      {"d_offsets", &Args::d_offsets, 8},         {"d_levels", &Args::d_levels, 16},
                            {"d_keep", &Args::d_keep, 8},
                            {"d_add", &Args::d_add, 16},            {"d_add_offsets", &Args::d_add_offsets, 8}, {"d_leaves_new", &Args::d_leaves_new, 16},
                            {"d_offsets_new", &Args::d_offsets_new, 8}, {"d_levels_new", &Args::d_levels_new, 16},  {"d_roots", &Args::d_roots, 16},
                            {"d_n_bad", &Args::d_n_bad, 4},         {"d_n_hashed", &Args::d_n_hashed, 8}};
        null_and_misaligned(cases, bufs);
        // every output range against every input range: the output starts inside the input's last 16 bytes, and just behind the input
        const struct {
            const char* name;
            uint64_t Args::*at;
            uint64_t bytes;
        } ins[] = {{"d_leaves", &Args::d_leaves, 12 * 32}, {"d_offsets", &Args::d_offsets, 4 * 8}, {"d_levels", &Args::d_levels, (12 / (arity - 1) + 3 * (arity == 4 ? 2u : 3u)) * 32},
                   {"d_add", &Args::d_add, 6 * 32},        {"d_add_offsets", &Args::d_add_offsets, 5 * 8}, {"d_keep", &Args::d_keep, 4 * 8}};
        const Buf outs[] = {{"d_leaves_new", &Args::d_leaves_new, 16}, {"d_offsets_new", &Args::d_offsets_new, 8}, {"d_levels_new", &Args::d_levels_new, 16},
                            {"d_roots", &Args::d_roots, 16},           {"d_n_bad", &Args::d_n_bad, 4},             {"d_n_hashed", &Args::d_n_hashed, 8}};
        for (const Buf& o : outs)
            for (const auto& i : ins) {
                const uint64_t Args::*in_at = i.at;
                const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;  // (multiples of 16: aligned for every output)
                cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Args& a) { a.*(o.at) = a.*in_at + last; }});
                cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Args& a) { a.*(o.at) = a.*in_at + in_bytes; }});
            }
        // an output that ends inside an input, and one that ends where it begins
        cases.push_back({"d_roots=d_add-16", [](Args& a) { a.d_roots = a.d_add - 16; }});
        cases.push_back({"d_roots=d_add-4*32", [](Args& a) { a.d_roots = a.d_add - 4 * 32; }});
        cases.push_back({"d_leaves_new=d_leaves-leaves_cap*32+16", [](Args& a) { a.d_leaves_new = a.d_leaves - 18 * 32 + 16; }});
        cases.push_back({"d_leaves_new=d_leaves-leaves_cap*32", [](Args& a) { a.d_leaves_new = a.d_leaves - 18 * 32; }});
        cases.push_back({"n_add=0,d_leaves_new=d_add", [](Args& a) { a.n_add = 0, a.d_leaves_new = a.d_add; }});  // (no byte of d_add is read)
        run_cases(sym, good, cases, [arity](const Args& a) { return call(arity, a); });
    }
    delete ctx;
    return 0;
}
