// refusal_table.hpp — the harness of the refusal programs (api_refusals.cpp, journal_refusals.cpp, append_refusals.cpp,
// resize_refusals.cpp, select_refusals.cpp, forest_multiproof_refusals.cpp and the frontier_, witness_ and
// consistency_refusal_table.cpp): each prints the argument refusals of its entry points as a table,
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before an entry point binds its device, so ONE context that never saw a device (device = -1) reaches all of
// them on a machine with or without a GPU.  The control row of an entry point — an all-good argument set — must get past validation
// and fail at hipSetDevice(ctx->device) with P252_ERR_HIP; every other row varies the control one way.  No pointer is dereferenced:
// no row reaches a device.  The case tables and the adapters that call the library stay in the programs; two styles of table share
// this file: the one of api_refusals.cpp (Arg / Combo / Entry: arguments by kind, varied one at a time) and the one of
// append_refusals.cpp and select_refusals.cpp (a struct of named arguments, CaseOf / BufOf: each case a function that changes the
// control).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../../poseidon252_amd/csrc/ctx.hpp"

namespace refusal {

inline uint64_t g_tag[4] = {1, 2, 3, 4};
inline const uint64_t MAXZ = SIZE_MAX;

inline p252_ctx* C(uint64_t v) { return reinterpret_cast<p252_ctx*>(v); }
inline void* P(uint64_t v) { return reinterpret_cast<void*>(v); }
inline const uint64_t* T(uint64_t v) { return reinterpret_cast<const uint64_t*>(v); }

inline void print_row(const char* sym, const std::string& what, int rc, std::string msg) {
    for (char& c : msg)
        if (c == '\t' || c == '\n') c = ' ';
    std::printf("%s\t%s\t%d\t%s\n", sym, what.c_str(), rc, msg.c_str());
}

// ---------------------------------------------------------------------------------------------- a struct of named arguments
// A: the program's struct, whose first member is `p252_ctx* ctx` and whose buffers are uint64_t addresses that nothing dereferences
inline uint64_t slot(unsigned i) { return 0x100000000ull + 0x100000ull * i; }  // 1 MiB apart

template <class A>
struct CaseOf {
    std::string name;
    std::function<void(A&)> vary;
};

template <class A>
struct BufOf {
    const char* name;
    uint64_t A::*at;
    unsigned align;
};

// every buffer NULL, and off by half its alignment
template <class A, size_t N>
void null_and_misaligned(std::vector<CaseOf<A>>& cases, const BufOf<A> (&bufs)[N]) {
    for (const BufOf<A>& b : bufs) {
        cases.push_back({std::string(b.name) + "=NULL", [b](A& a) { a.*(b.at) = 0; }});
        if (b.align > 1) cases.push_back({std::string(b.name) + "+" + std::to_string(b.align / 2), [b](A& a) { a.*(b.at) += b.align / 2; }});
    }
}

template <class A, class F>
void run_cases(const std::string& sym, const A& good, const std::vector<CaseOf<A>>& cases, F call) {
    for (const CaseOf<A>& c : cases) {
        A a = good;
        c.vary(a);
        good.ctx->err.clear();
        const int rc = call(a);
        print_row(sym.c_str(), c.name, rc, p252_last_error(a.ctx));
    }
}

// ---------------------------------------------------------------------------------------------- arguments by kind
alignas(64) inline unsigned char g_buf[64 * 32];
inline p252_ctx* g_ctx = nullptr;

enum Kind {
    CTX,   // the context
    HOST,  // a host pointer the library reads at once (tag, arrays of the multi calls): NULL only
    P16,   // device scalar array: NULL, +8
    P8,    // device uint64 array: NULL, +4
    P4,    // device uint32 array: NULL, +2
    P1,    // device byte array: NULL
    CNT,   // size_t count: 0, the common edges, its own edges
    INT,   // int / unsigned selector: its own edges only
};

struct Arg {
    const char* name;
    Kind kind;
    uint64_t good;                // CNT / INT: the good value; pointers: filled in (a slot of g_buf)
    std::vector<uint64_t> edges;  // further values of this argument
};

struct Combo {  // several arguments at once: overflow products, "NULL is fine when the count is 0"
    const char* name;
    std::vector<std::pair<const char*, uint64_t>> set;
};

using V = const uint64_t*;
struct Entry {
    const char* sym;
    std::vector<Arg> args;
    std::function<int(V)> call;
    std::vector<Combo> combos;
    bool ctx_array = false;  // slot 0 is an array of contexts (the multi calls): the message is the one context's
};

inline const std::vector<uint64_t> COMMON = {MAXZ, 1ull << 32, (1ull << 32) - 1, 0x80000000ull, 0x7fffffffull};

inline std::string hex(uint64_t v) {
    char b[32];
    std::snprintf(b, sizeof b, v < 10 ? "%llu" : "0x%llx", (unsigned long long)v);
    return b;
}

inline void row(const Entry& e, const std::string& what, const std::vector<uint64_t>& v) {
    g_ctx->err.clear();
    const int rc = e.call(v.data());
    print_row(e.sym, what, rc, p252_last_error(e.ctx_array ? g_ctx : C(v[0])));
}

// the all-good argument set of the control row (fills in the pointers' good values)
inline std::vector<uint64_t> good_values(Entry& e) {
    std::vector<uint64_t> good;
    for (size_t i = 0; i < e.args.size(); ++i) {
        Arg& a = e.args[i];
        if (a.kind == CTX) a.good = reinterpret_cast<uint64_t>(g_ctx);
        if (a.kind == HOST && !a.good) a.good = reinterpret_cast<uint64_t>(g_tag);
        if (a.kind == P16 || a.kind == P8 || a.kind == P4 || a.kind == P1) a.good = reinterpret_cast<uint64_t>(g_buf + 64 * (i + 1));
        good.push_back(a.good);
    }
    return good;
}

inline void run(Entry& e) {
    const std::vector<uint64_t> good = good_values(e);
    row(e, "control", good);
    for (size_t i = 0; i < e.args.size(); ++i) {
        const Arg& a = e.args[i];
        auto vary = [&](const std::string& what, uint64_t val) {
            std::vector<uint64_t> v = good;
            v[i] = val;
            row(e, std::string(a.name) + what, v);
        };
        if (a.kind != CNT && a.kind != INT) vary("=NULL", 0);
        if (a.kind == P16) vary("+8", a.good + 8);
        if (a.kind == P8) vary("+4", a.good + 4);
        if (a.kind == P4) vary("+2", a.good + 2);
        if (a.kind == CNT) {
            vary("=0", 0);
            for (uint64_t x : COMMON) vary("=" + hex(x), x);
        }
        for (uint64_t x : a.edges) vary("=" + hex(x), x);
    }
    for (const Combo& c : e.combos) {
        std::vector<uint64_t> v = good;
        for (const auto& s : c.set) {
            size_t i = 0;
            while (i < e.args.size() && std::string(e.args[i].name) != s.first) ++i;
            if (i == e.args.size()) {
                std::fprintf(stderr, "%s: combo %s names no argument %s\n", e.sym, c.name, s.first);
                std::exit(2);
            }
            v[i] = s.second;
        }
        row(e, c.name, v);
    }
}

// The ORDER of an entry point's checks, which rows that vary one argument cannot show: for every unordered pair of its arguments, both
// varied at once — a pointer NULL and (where it has an alignment) off by half of it, a count 0 and SIZE_MAX, a selector at its own
// edges — in every combination.  The row names the check that fails first.  Two libraries agree on the order of their checks when
// they print the same rows; nothing records these (a program's --pairs mode prints them).
inline std::vector<std::pair<std::string, uint64_t>> pair_variants(const Arg& a) {
    std::vector<std::pair<std::string, uint64_t>> vs;
    if (a.kind != CNT && a.kind != INT) vs.push_back({"=NULL", 0});
    if (a.kind == P16) vs.push_back({"+8", a.good + 8});
    if (a.kind == P8) vs.push_back({"+4", a.good + 4});
    if (a.kind == P4) vs.push_back({"+2", a.good + 2});
    if (a.kind == CNT) vs.insert(vs.end(), {{"=0", 0}, {"=SIZE_MAX", MAXZ}});
    if (a.kind == INT)
        for (uint64_t x : a.edges) vs.push_back({"=" + hex(x), x});
    return vs;
}

inline void run_pairs(Entry& e) {
    const std::vector<uint64_t> good = good_values(e);
    for (size_t i = 0; i < e.args.size(); ++i)
        for (size_t j = i + 1; j < e.args.size(); ++j)
            for (const auto& x : pair_variants(e.args[i]))
                for (const auto& y : pair_variants(e.args[j])) {
                    std::vector<uint64_t> v = good;
                    v[i] = x.second, v[j] = y.second;
                    row(e, e.args[i].name + x.first + "," + e.args[j].name + y.first, v);
                }
}

inline const Arg CTXA = {"ctx", CTX, 0, {}}, TAGA = {"tag", HOST, 0, {}};
inline Arg cnt(const char* name, uint64_t good, std::vector<uint64_t> edges = {}) { return {name, CNT, good, edges}; }
inline Arg p16(const char* name) { return {name, P16, 0, {}}; }
inline Arg p8(const char* name) { return {name, P8, 0, {}}; }
inline Arg p4(const char* name) { return {name, P4, 0, {}}; }
inline Arg p1(const char* name) { return {name, P1, 0, {}}; }

// limits of the library's size checks (api_forest.cpp): forest_shape_check, the `k > SIZE_MAX / 128 / depth` family, the ragged depths
inline const uint64_t FOREST_MAX_DEPTH = 64;  // FOREST_RAGGED_MAX_DEPTH = FOREST_OPENINGS_MAX_DEPTH
inline const uint64_t TREES_MAX = MAXZ / 8 / (FOREST_MAX_DEPTH + 2);

inline std::vector<Combo> forest_shape_combos() {
    return {{"n_leaves=SIZE_MAX/64", {{"n_leaves", MAXZ / 64}}},
            {"n_leaves=SIZE_MAX/64+1", {{"n_leaves", MAXZ / 64 + 1}}},
            {"n_trees=SIZE_MAX/8/66", {{"n_trees", TREES_MAX}}},
            {"n_trees=SIZE_MAX/8/66+1", {{"n_trees", TREES_MAX + 1}}},
            {"n_trees*min(max_leaves,n_leaves)=SIZE_MAX/2", {{"n_leaves", 1ull << 40}, {"max_leaves", 1ull << 41}, {"n_trees", (MAXZ / 2) >> 40}}},
            {"n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2", {{"n_leaves", 1ull << 40}, {"max_leaves", 1ull << 41}, {"n_trees", ((MAXZ / 2) >> 40) + 1}}},
            {"n_trees*max_leaves>SIZE_MAX/2,max_leaves<n_leaves", {{"n_leaves", 1ull << 50}, {"max_leaves", 1ull << 40}, {"n_trees", ((MAXZ / 2) >> 40) + 1}}}};
}

}  // namespace refusal
