// frontier_refusal_table.cpp — the argument refusals of p252_merkle{4,2}_forest_frontier_append_device_into and
// p252_merkle{4,2}_forest_frontier_extract_device_into, and the values of p252_merkle{4,2}_forest_frontier_bound, as a table in the
// format of api_refusals.cpp:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_forest_frontier_cpu.py compares the lines with tests/golden/frontier_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Append {
    p252_ctx* ctx;
    const uint64_t* tag;
    uint64_t d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, n_add, d_add_offsets, d_n_bad, d_n_hashed;
};

int call(unsigned arity, const Append& a) {
    return (arity == 4 ? p252_merkle4_forest_frontier_append_device_into : p252_merkle2_forest_frontier_append_device_into)(
        a.ctx, a.tag, P(a.d_counts), P(a.d_frontier), P(a.d_roots), a.n_trees, a.max_leaves, P(a.d_add), a.n_add, P(a.d_add_offsets), P(a.d_n_bad),
        P(a.d_n_hashed), nullptr);
}

struct Extract {
    p252_ctx* ctx;
    uint64_t d_leaves, n_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots_forest, max_leaves, d_counts, d_frontier, d_roots, d_n_bad;
};

int call(unsigned arity, const Extract& a) {
    return (arity == 4 ? p252_merkle4_forest_frontier_extract_device_into : p252_merkle2_forest_frontier_extract_device_into)(
        a.ctx, P(a.d_leaves), a.n_leaves, P(a.d_offsets), a.n_trees, a.max_leaves_forest, P(a.d_levels), P(a.d_roots_forest), a.max_leaves,
        P(a.d_counts), P(a.d_frontier), P(a.d_roots), P(a.d_n_bad), nullptr);
}

void bounds(unsigned arity) {
    const char* sym = arity == 4 ? "p252_merkle4_forest_frontier_bound" : "p252_merkle2_forest_frontier_bound";
    for (uint64_t n : std::vector<uint64_t>{0, 1, 2, 3, 4, 5, 16, 17, 1ull << 24, (1ull << 24) + 1, 1ull << 32, MAXZ}) {
        const size_t b = arity == 4 ? p252_merkle4_forest_frontier_bound(n) : p252_merkle2_forest_frontier_bound(n);
        print_row(sym, "max_leaves=" + hex(n), (int)b, "");
    }
}

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (unsigned arity : {4u, 2u}) {
        bounds(arity);
        {
            const char* sym = arity == 4 ? "p252_merkle4_forest_frontier_append_device_into" : "p252_merkle2_forest_frontier_append_device_into";
            // 5 trees of at most 100 leaves (depth 4 / 7: 15 / 8 scalars of frontier each) receive 12 leaves
            const uint64_t stride = arity == 4 ? 15 : 8;
            const Append good = {ctx, g_tag, slot(0), slot(1), slot(2), 5, 100, slot(3), 12, slot(4), slot(5), slot(6)};
            using Case = CaseOf<Append>;
            using Buf = BufOf<Append>;
            std::vector<Case> cases = {
                {"control", [](Append&) {}},
                {"ctx=NULL", [](Append& a) { a.ctx = nullptr; }},
                {"tag=NULL", [](Append& a) { a.tag = nullptr; }},
                {"n_trees=0", [](Append& a) { a.n_trees = 0; }},
                {"n_trees=0,max_leaves=0", [](Append& a) { a.n_trees = a.max_leaves = 0; }},
                {"max_leaves=0", [](Append& a) { a.max_leaves = 0; }},
                {"max_leaves=1", [](Append& a) { a.max_leaves = 1; }},
                {"max_leaves=SIZE_MAX", [](Append& a) { a.max_leaves = MAXZ; }},
                {"n_add=0", [](Append& a) { a.n_add = 0; }},
                {"n_add=0,d_add=NULL", [](Append& a) { a.n_add = 0, a.d_add = 0; }},
                {"n_add=2^32-1", [](Append& a) { a.n_add = 0xffffffffull, a.d_add = 1ull << 50; }},  // (128 GiB of d_add, clear of the other buffers)
                {"n_add=2^32", [](Append& a) { a.n_add = 1ull << 32; }},
                {"n_add=SIZE_MAX", [](Append& a) { a.n_add = MAXZ; }},
                {"n_trees=SIZE_MAX/8/66+1", [](Append& a) { a.n_trees = TREES_MAX + 1; }},
                {"n_trees=SIZE_MAX/64/bound+1", [stride](Append& a) { a.n_trees = MAXZ / 64 / stride + 1; }},
                {"n_trees*n_add>SIZE_MAX/2", [](Append& a) { a.n_add = 1ull << 31, a.n_trees = ((MAXZ / 2) >> 31) + 1, a.max_leaves = 1; }},
            };
            const Buf bufs[] = {{"d_counts", &Append::d_counts, 8},     {"d_frontier", &Append::d_frontier, 16}, {"d_roots", &Append::d_roots, 16},
                                {"d_add", &Append::d_add, 16},          {"d_add_offsets", &Append::d_add_offsets, 8},
                                {"d_n_bad", &Append::d_n_bad, 4},       {"d_n_hashed", &Append::d_n_hashed, 8}};
            null_and_misaligned(cases, bufs);
            // the state and the counters against the two inputs: inside the input's last 16 bytes, and just behind it
            const struct {
                const char* name;
                uint64_t Append::*at;
                uint64_t bytes;
            } ins[] = {{"d_add", &Append::d_add, 12 * 32}, {"d_add_offsets", &Append::d_add_offsets, 6 * 8}};
            const Buf outs[] = {{"d_counts", &Append::d_counts, 8}, {"d_frontier", &Append::d_frontier, 16}, {"d_roots", &Append::d_roots, 16},
                                {"d_n_bad", &Append::d_n_bad, 4},   {"d_n_hashed", &Append::d_n_hashed, 8}};
            for (const Buf& o : outs)
                for (const auto& i : ins) {
                    const uint64_t Append::*in_at = i.at;
                    const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;
                    cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Append& a) { a.*(o.at) = a.*in_at + last; }});
                    cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Append& a) { a.*(o.at) = a.*in_at + in_bytes; }});
                }
            // the frontier ends inside d_add, and where d_add begins
            cases.push_back({"d_frontier=d_add-bytes+16", [stride](Append& a) { a.d_frontier = a.d_add - 5 * stride * 32 + 16; }});
            cases.push_back({"d_frontier=d_add-bytes", [stride](Append& a) { a.d_frontier = a.d_add - 5 * stride * 32; }});
            cases.push_back({"n_add=0,d_roots=d_add", [](Append& a) { a.n_add = 0, a.d_roots = a.d_add; }});  // (no byte of d_add is read)
            run_cases(sym, good, cases, [arity](const Append& a) { return call(arity, a); });
        }
        {
            const char* sym = arity == 4 ? "p252_merkle4_forest_frontier_extract_device_into" : "p252_merkle2_forest_frontier_extract_device_into";
            // a forest of 3 trees of at most 5 of 12 leaves, into a state for trees of at most 100
            const Extract good = {ctx, slot(0), 12, slot(1), 3, 5, slot(2), slot(3), 100, slot(4), slot(5), slot(6), slot(7)};
            using Case = CaseOf<Extract>;
            using Buf = BufOf<Extract>;
            std::vector<Case> cases = {
                {"control", [](Extract&) {}},
                {"ctx=NULL", [](Extract& a) { a.ctx = nullptr; }},
                {"n_trees=0", [](Extract& a) { a.n_trees = 0; }},
                {"max_leaves_forest=0", [](Extract& a) { a.max_leaves_forest = 0; }},
                {"max_leaves=max_leaves_forest-1", [](Extract& a) { a.max_leaves = 4; }},
                {"max_leaves=max_leaves_forest", [](Extract& a) { a.max_leaves = 5; }},
                {"max_leaves_forest=1,d_levels=NULL", [](Extract& a) { a.max_leaves_forest = 1, a.d_levels = 0; }},
                {"n_leaves=SIZE_MAX/64+1", [](Extract& a) { a.n_leaves = MAXZ / 64 + 1; }},
                {"n_trees=SIZE_MAX/8/66+1", [](Extract& a) { a.n_trees = TREES_MAX + 1; }},
            };
            const Buf bufs[] = {{"d_leaves", &Extract::d_leaves, 16},   {"d_offsets", &Extract::d_offsets, 8},
                                {"d_levels", &Extract::d_levels, 16},   {"d_roots_forest", &Extract::d_roots_forest, 16},
                                {"d_counts", &Extract::d_counts, 8},    {"d_frontier", &Extract::d_frontier, 16},
                                {"d_roots", &Extract::d_roots, 16},     {"d_n_bad", &Extract::d_n_bad, 4}};
            null_and_misaligned(cases, bufs);
            const struct {
                const char* name;
                uint64_t Extract::*at;
                uint64_t bytes;
            } ins[] = {{"d_leaves", &Extract::d_leaves, 12 * 32},
                       {"d_offsets", &Extract::d_offsets, 4 * 8},
                       {"d_levels", &Extract::d_levels, (12 / (arity - 1) + 3 * (arity == 4 ? 2u : 3u)) * 32},
                       {"d_roots_forest", &Extract::d_roots_forest, 3 * 32}};
            const Buf outs[] = {{"d_counts", &Extract::d_counts, 8}, {"d_frontier", &Extract::d_frontier, 16}, {"d_roots", &Extract::d_roots, 16},
                                {"d_n_bad", &Extract::d_n_bad, 4}};
            for (const Buf& o : outs)
                for (const auto& i : ins) {
                    const uint64_t Extract::*in_at = i.at;
                    const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;
                    cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Extract& a) { a.*(o.at) = a.*in_at + last; }});
                    cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Extract& a) { a.*(o.at) = a.*in_at + in_bytes; }});
                }
            run_cases(sym, good, cases, [arity](const Extract& a) { return call(arity, a); });
        }
    }
    delete ctx;
    return 0;
}
