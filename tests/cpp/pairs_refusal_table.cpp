// pairs_refusal_table.cpp — the argument refusals of p252_pairs_order_device_into and p252_pairs_unique_device_into, as a table in the
// format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_pairs_order_cpu.py compares the lines with tests/golden/pairs_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

struct Args {
    p252_ctx* ctx;
    uint64_t d_tree_ids, d_leaf_ids, k, d_order, d_tree_ids_out, d_leaf_ids_out, d_indices_out, d_first, d_n_unique;
};

int order(const Args& a) { return p252_pairs_order_device_into(a.ctx, P(a.d_tree_ids), P(a.d_leaf_ids), a.k, P(a.d_order), nullptr); }
int unique(const Args& a) {
    return p252_pairs_unique_device_into(a.ctx, P(a.d_tree_ids), P(a.d_leaf_ids), a.k, P(a.d_tree_ids_out), P(a.d_leaf_ids_out),
                                         P(a.d_indices_out), P(a.d_first), P(a.d_n_unique), nullptr);
}

using Case = CaseOf<Args>;
using Buf = BufOf<Args>;

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    // 9 pairs: every array far inside its 1 MiB
    const Args good = {ctx, slot(0), slot(1), 9, slot(2), slot(3), slot(4), slot(5), slot(6), slot(7)};
    const std::vector<Case> counts = {
        {"control", [](Args&) {}},
        {"ctx=NULL", [](Args& a) { a.ctx = nullptr; }},
        {"k=0", [](Args& a) { a.k = 0; }},
        {"k=1", [](Args& a) { a.k = 1; }},
        {"k=2^32-1", [](Args& a) { a.k = 0xffffffffull; }},
        {"k=2^32", [](Args& a) { a.k = 1ull << 32; }},
        {"k=SIZE_MAX/16+1", [](Args& a) { a.k = MAXZ / 16 + 1; }},  // (a size that would overflow is at or past 2^32)
        {"k=SIZE_MAX", [](Args& a) { a.k = MAXZ; }},
    };
    {
        std::vector<Case> cases = counts;
        cases.push_back({"d_order=d_tree_ids", [](Args& a) { a.d_order = a.d_tree_ids; }});
        cases.push_back({"d_order=d_leaf_ids+8", [](Args& a) { a.d_order = a.d_leaf_ids + 8; }});
        cases.push_back({"d_order=d_leaf_ids+8*8", [](Args& a) { a.d_order = a.d_leaf_ids + 8 * 8; }});
        cases.push_back({"d_order=d_leaf_ids+8*9", [](Args& a) { a.d_order = a.d_leaf_ids + 8 * 9; }});
        cases.push_back({"d_tree_ids=NULL,d_order=d_leaf_ids", [](Args& a) { a.d_tree_ids = 0, a.d_order = a.d_leaf_ids; }});
        const Buf bufs[] = {{"d_tree_ids", &Args::d_tree_ids, 4}, {"d_leaf_ids", &Args::d_leaf_ids, 8}, {"d_order", &Args::d_order, 4}};
        null_and_misaligned(cases, bufs);
        run_cases("p252_pairs_order_device_into", good, cases, order);
    }
    {
        std::vector<Case> cases = counts;
        cases.push_back({"one output: d_first", [](Args& a) { a.d_tree_ids_out = a.d_leaf_ids_out = a.d_indices_out = 0; }});
        cases.push_back({"one output: d_indices_out", [](Args& a) { a.d_tree_ids_out = a.d_leaf_ids_out = a.d_first = 0; }});
        cases.push_back({"no array output", [](Args& a) { a.d_tree_ids_out = a.d_leaf_ids_out = a.d_indices_out = a.d_first = 0; }});
        cases.push_back({"d_tree_ids_out=d_tree_ids", [](Args& a) { a.d_tree_ids_out = a.d_tree_ids; }});
        cases.push_back({"d_leaf_ids_out=d_leaf_ids+8", [](Args& a) { a.d_leaf_ids_out = a.d_leaf_ids + 8; }});
        cases.push_back({"d_indices_out=d_leaf_ids", [](Args& a) { a.d_indices_out = a.d_leaf_ids; }});
        cases.push_back({"d_first=d_tree_ids+4", [](Args& a) { a.d_first = a.d_tree_ids + 4; }});
        cases.push_back({"d_n_unique=d_leaf_ids+8", [](Args& a) { a.d_n_unique = a.d_leaf_ids + 8; }});
        cases.push_back({"d_first=d_indices_out", [](Args& a) { a.d_first = a.d_indices_out; }});
        cases.push_back({"d_leaf_ids_out=d_tree_ids_out+8", [](Args& a) { a.d_leaf_ids_out = a.d_tree_ids_out + 8; }});
        cases.push_back({"d_n_unique=d_first+8", [](Args& a) { a.d_n_unique = a.d_first + 8; }});
        cases.push_back({"d_n_unique=d_first+4*8", [](Args& a) { a.d_n_unique = a.d_first + 4 * 8; }});
        cases.push_back({"d_n_unique=d_first+4*10", [](Args& a) { a.d_n_unique = a.d_first + 4 * 10; }});
        const Buf bufs[] = {{"d_tree_ids", &Args::d_tree_ids, 4},         {"d_leaf_ids", &Args::d_leaf_ids, 8},
                            {"d_tree_ids_out", &Args::d_tree_ids_out, 4}, {"d_leaf_ids_out", &Args::d_leaf_ids_out, 8},
                            {"d_indices_out", &Args::d_indices_out, 4},   {"d_first", &Args::d_first, 4},
                            {"d_n_unique", &Args::d_n_unique, 8}};
        null_and_misaligned(cases, bufs);
        run_cases("p252_pairs_unique_device_into", good, cases, unique);
    }
    delete ctx;
    return 0;
}
