// select_refusals.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_select_device_into, as a table, in the format of
// api_refusals.cpp:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_select_cpu.py compares the lines with tests/golden/select_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    uint64_t d_leaves_a, n_leaves_a, d_offsets_a, n_trees_a, max_leaves_a, d_levels_a, d_roots_a, d_leaves_b, n_leaves_b, d_offsets_b, n_trees_b,
        max_leaves_b, d_levels_b, d_roots_b, d_pick, n_pick, d_leaves_new, leaves_cap, d_offsets_new, d_levels_new, levels_cap, d_roots_new, d_n_bad;
};

int call(unsigned arity, const Args& a) {
    return (arity == 4 ? p252_merkle4_forest_ragged_select_device_into : p252_merkle2_forest_ragged_select_device_into)(
        a.ctx, P(a.d_leaves_a), a.n_leaves_a, P(a.d_offsets_a), a.n_trees_a, a.max_leaves_a, P(a.d_levels_a), P(a.d_roots_a), P(a.d_leaves_b),
        a.n_leaves_b, P(a.d_offsets_b), a.n_trees_b, a.max_leaves_b, P(a.d_levels_b), P(a.d_roots_b), P(a.d_pick), a.n_pick, P(a.d_leaves_new),
        a.leaves_cap, P(a.d_offsets_new), P(a.d_levels_new), a.levels_cap, P(a.d_roots_new), P(a.d_n_bad), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

struct Range {
    const char* name;
    uint64_t Args::*at;
    uint64_t bytes;
};

// the three sizes of one forest of the call, under the names forest_shape_combos() uses
struct Shape {
    const char* who;
    uint64_t Args::*n_leaves;
    uint64_t Args::*n_trees;
    uint64_t Args::*max_leaves;
};

void shape_edges(std::vector<Case>& cases, const Shape& s) {
    for (const Combo& c : forest_shape_combos()) {
        std::vector<std::pair<uint64_t Args::*, uint64_t>> set;
        for (const auto& kv : c.set) {
            const std::string field = kv.first;
            set.push_back({field == "n_leaves" ? s.n_leaves : field == "n_trees" ? s.n_trees : s.max_leaves, kv.second});
        }
        cases.push_back({std::string(s.who) + ":" + c.name, [set](Args& a) {
                             for (const auto& kv : set) a.*(kv.first) = kv.second;
                         }});
    }
}

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        const char* sym = arity == 4 ? "p252_merkle4_forest_ragged_select_device_into" : "p252_merkle2_forest_ragged_select_device_into";
        // A: 2 trees of at most 9 of 16 leaves; B: 3 trees of at most 12 of 24 leaves; 4 picks into room for 30 leaves
        const uint64_t per = arity - 1, D = arity == 4 ? 2 : 4, D17 = arity == 4 ? 3 : 5;  // depth(9) = depth(12) = D, depth(17) = D17
        const uint64_t need = 30 / per + 4 * D, need17 = 30 / per + 4 * D17;
        const Args good = {ctx,     slot(0), 16,      slot(1), 2, 9,       slot(2), slot(3), slot(4),  24,       slot(5),  3,
                           12,      slot(6), slot(7), slot(8), 4, slot(9), 30,      slot(10), slot(11), need,     slot(12), slot(13)};
        std::vector<Case> cases = {
            {"control", [](Args&) {}},
            {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
            // the sizes
            {"n_trees_a=0", [](Args& a) { a.n_trees_a = 0; }},
            {"n_pick=0", [](Args& a) { a.n_pick = 0; }},
            {"n_pick=0,n_leaves_a=0,buffers=NULL",
             [ctx](Args& a) { a = Args{ctx, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }},
            // B absent: nothing of it is looked at
            {"n_trees_b=0,B=NULL", [](Args& a) { a.n_trees_b = a.n_leaves_b = a.max_leaves_b = a.d_leaves_b = a.d_offsets_b = a.d_levels_b = a.d_roots_b = 0; }},
            {"n_trees_b=0", [](Args& a) { a.n_trees_b = 0; }},
            {"n_trees_b=0,B misaligned", [](Args& a) { a.n_trees_b = 0, a.d_leaves_b += 8, a.d_offsets_b += 4, a.d_levels_b += 8, a.d_roots_b += 8; }},
            {"n_trees_b=0,B on the outputs",
             [](Args& a) { a.n_trees_b = 0, a.d_leaves_b = a.d_leaves_new, a.d_offsets_b = a.d_offsets_new, a.d_levels_b = a.d_levels_new, a.d_roots_b = a.d_roots_new; }},
            {"n_trees_b=0,n_leaves_b=0,max_leaves_b=0", [](Args& a) { a.n_trees_b = a.n_leaves_b = a.max_leaves_b = 0; }},
            {"n_leaves_b=0", [](Args& a) { a.n_leaves_b = 0; }},
            {"max_leaves_b=0", [](Args& a) { a.max_leaves_b = 0; }},
            {"n_leaves_a=0", [](Args& a) { a.n_leaves_a = 0; }},
            {"max_leaves_a=0", [](Args& a) { a.max_leaves_a = 0; }},
            {"leaves_cap=0", [](Args& a) { a.leaves_cap = 0; }},
            // the levels' cap: leaves_cap / (arity - 1) + n_pick * depth(max(max_leaves_a, max_leaves_b))
            {"levels_cap=need-1", [need](Args& a) { a.levels_cap = need - 1; }},
            {"levels_cap=need", [need](Args& a) { a.levels_cap = need; }},
            {"levels_cap=need+1", [need](Args& a) { a.levels_cap = need + 1; }},
            {"levels_cap=0", [](Args& a) { a.levels_cap = 0; }},
            {"max_leaves_a=17", [](Args& a) { a.max_leaves_a = 17; }},
            {"max_leaves_a=17,levels_cap=need(17)-1", [need17](Args& a) { a.max_leaves_a = 17, a.levels_cap = need17 - 1; }},
            {"max_leaves_a=17,levels_cap=need(17)", [need17](Args& a) { a.max_leaves_a = 17, a.levels_cap = need17; }},
            {"max_leaves_b=17,levels_cap=need(17)-1", [need17](Args& a) { a.max_leaves_b = 17, a.levels_cap = need17 - 1; }},
            {"max_leaves_b=17,levels_cap=need(17)", [need17](Args& a) { a.max_leaves_b = 17, a.levels_cap = need17; }},
            {"n_trees_b=0,max_leaves_b=17", [](Args& a) { a.n_trees_b = 0, a.max_leaves_b = 17; }},  // (B absent: its max_leaves does not count)
            // one-leaf trees have no levels
            {"max_leaves_a=1,d_levels_a=NULL", [](Args& a) { a.max_leaves_a = 1, a.d_levels_a = 0; }},
            {"max_leaves_a=2,d_levels_a=NULL", [](Args& a) { a.max_leaves_a = 2, a.d_levels_a = 0; }},
            {"max_leaves_b=1,d_levels_b=NULL", [](Args& a) { a.max_leaves_b = 1, a.d_levels_b = 0; }},
            {"max_leaves_a=1,d_levels_new=NULL", [](Args& a) { a.max_leaves_a = 1, a.d_levels_new = 0; }},
            {"max_leaves_a=max_leaves_b=1,levels=NULL",
             [](Args& a) { a.max_leaves_a = a.max_leaves_b = 1, a.d_levels_a = a.d_levels_b = a.d_levels_new = 0; }},
            // overflow (each forest alone is bounded by the shape check, so the sum of the two tree counts never wraps behind it)
            {"n_trees_a=SIZE_MAX,n_trees_b=1", [](Args& a) { a.n_trees_a = MAXZ, a.n_trees_b = 1; }},
            {"n_trees_a=n_trees_b=SIZE_MAX/2+1", [](Args& a) { a.n_trees_a = a.n_trees_b = MAXZ / 2 + 1; }},
            {"n_pick*min(max_leaves_a,n_leaves_a)=SIZE_MAX/2",
             [](Args& a) { a.n_leaves_a = 1ull << 40, a.max_leaves_a = 1ull << 41, a.n_pick = (MAXZ / 2) >> 40; }},
            {"n_pick*min(max_leaves_a,n_leaves_a)>SIZE_MAX/2",
             [](Args& a) { a.n_leaves_a = 1ull << 40, a.max_leaves_a = 1ull << 41, a.n_pick = ((MAXZ / 2) >> 40) + 1; }},
            {"n_pick*min(max_leaves_b,n_leaves_b)>SIZE_MAX/2",
             [](Args& a) { a.n_leaves_b = 1ull << 40, a.max_leaves_b = 1ull << 41, a.n_pick = ((MAXZ / 2) >> 40) + 1; }},
            {"n_trees_b=0,n_pick*min(max_leaves_b,n_leaves_b)>SIZE_MAX/2",
             [](Args& a) { a.n_trees_b = 0, a.n_leaves_b = 1ull << 40, a.max_leaves_b = 1ull << 41, a.n_pick = ((MAXZ / 2) >> 40) + 1; }},
            {"levels_cap=SIZE_MAX/64", [](Args& a) { a.levels_cap = MAXZ / 64; }},
            {"levels_cap=SIZE_MAX/64+1", [](Args& a) { a.levels_cap = MAXZ / 64 + 1; }},
            {"levels_cap=SIZE_MAX", [](Args& a) { a.levels_cap = MAXZ; }},
        };
        shape_edges(cases, {"A", &Args::n_leaves_a, &Args::n_trees_a, &Args::max_leaves_a});
        shape_edges(cases, {"B", &Args::n_leaves_b, &Args::n_trees_b, &Args::max_leaves_b});
        shape_edges(cases, {"new", &Args::leaves_cap, &Args::n_pick, &Args::max_leaves_a});
        // every buffer NULL, and off its alignment
        const Buf bufs[] = {{"d_leaves_a", &Args::d_leaves_a, 16},     {"d_offsets_a", &Args::d_offsets_a, 8},     {"d_levels_a", &Args::d_levels_a, 16},
                            {"d_roots_a", &Args::d_roots_a, 16},       {"d_leaves_b", &Args::d_leaves_b, 16},      {"d_offsets_b", &Args::d_offsets_b, 8},
                            {"d_levels_b", &Args::d_levels_b, 16},     {"d_roots_b", &Args::d_roots_b, 16},        {"d_pick", &Args::d_pick, 8},
                            {"d_leaves_new", &Args::d_leaves_new, 16}, {"d_offsets_new", &Args::d_offsets_new, 8}, {"d_levels_new", &Args::d_levels_new, 16},
                            {"d_roots_new", &Args::d_roots_new, 16},   {"d_n_bad", &Args::d_n_bad, 4}};
        null_and_misaligned(cases, bufs);
        // every output against every input and every output before it: inside the other's last 16 bytes, and just behind it
        const Range ins[] = {{"d_leaves_a", &Args::d_leaves_a, 16 * 32},
                             {"d_offsets_a", &Args::d_offsets_a, 3 * 8},
                             {"d_levels_a", &Args::d_levels_a, (16 / per + 2 * D) * 32},
                             {"d_roots_a", &Args::d_roots_a, 2 * 32},
                             {"d_leaves_b", &Args::d_leaves_b, 24 * 32},
                             {"d_offsets_b", &Args::d_offsets_b, 4 * 8},
                             {"d_levels_b", &Args::d_levels_b, (24 / per + 3 * D) * 32},
                             {"d_roots_b", &Args::d_roots_b, 3 * 32},
                             {"d_pick", &Args::d_pick, 4 * 8}};
        const Range outs[] = {{"d_leaves_new", &Args::d_leaves_new, 30 * 32},
                              {"d_offsets_new", &Args::d_offsets_new, 5 * 8},
                              {"d_levels_new", &Args::d_levels_new, need * 32},
                              {"d_roots_new", &Args::d_roots_new, 4 * 32},
                              {"d_n_bad", &Args::d_n_bad, 4}};
        for (size_t x = 0; x < sizeof outs / sizeof *outs; ++x) {
            const Range o = outs[x];
            auto add = [&](const Range& i) {
                const uint64_t Args::*in_at = i.at;
                const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;  // (multiples of 16: aligned for every output)
                cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Args& a) { a.*(o.at) = a.*in_at + last; }});
                cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Args& a) { a.*(o.at) = a.*in_at + in_bytes; }});
            };
            for (const Range& i : ins) add(i);
            for (size_t y = 0; y < x; ++y) add(outs[y]);
        }
        // an output that ends inside an input, and one that ends where it begins; two outputs on one address
        cases.push_back({"d_roots_new=d_pick-16", [](Args& a) { a.d_roots_new = a.d_pick - 16; }});
        cases.push_back({"d_roots_new=d_pick-4*32", [](Args& a) { a.d_roots_new = a.d_pick - 4 * 32; }});
        cases.push_back({"d_leaves_new=d_leaves_b-leaves_cap*32+16", [](Args& a) { a.d_leaves_new = a.d_leaves_b - 30 * 32 + 16; }});
        cases.push_back({"d_leaves_new=d_leaves_b-leaves_cap*32", [](Args& a) { a.d_leaves_new = a.d_leaves_b - 30 * 32; }});
        cases.push_back({"d_leaves_new=d_levels_new", [](Args& a) { a.d_leaves_new = a.d_levels_new; }});
        // the ranges follow the sizes: the levels' cap beyond the bound is written too, a larger A is read to its end
        cases.push_back({"levels_cap=need+1,d_roots_new=d_levels_new+need*32", [need](Args& a) { a.levels_cap = need + 1, a.d_roots_new = a.d_levels_new + need * 32; }});
        cases.push_back({"d_roots_new=d_levels_new+need*32", [need](Args& a) { a.d_roots_new = a.d_levels_new + need * 32; }});
        run_cases(sym, good, cases, [arity](const Args& a) { return call(arity, a); });
    }
    delete ctx;
    return 0;
}
