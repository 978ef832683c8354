// journal_refusals.cpp — the argument refusals of p252_merkle{4,2}_forest_ragged_update_journaled_device_into and
// p252_merkle{4,2}_forest_ragged_journal_swap_device_into, as a table in the format of api_refusals.cpp, whose method this is:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so ONE context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  For each entry point the control row — an all-good argument set — must get past validation and fail
// at hipSetDevice(ctx->device) with P252_ERR_HIP; every other row varies one argument (ctx NULL, every pointer NULL, every aligned
// array off by half its alignment, every count at 0 and at both sides of every size check, the journal's capacity at both sides of the
// call's bound) or a named combination.  No pointer is dereferenced: no row reaches a device.
// (tests/test_forest_journal_cpu.py compares the lines with tests/golden/journal_refusals.txt.)
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../poseidon252_amd/csrc/ctx.hpp"

namespace {

alignas(64) unsigned char g_buf[64 * 32];
uint64_t g_tag[4] = {1, 2, 3, 4};

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

p252_ctx* g_ctx = nullptr;

p252_ctx* C(uint64_t v) { return reinterpret_cast<p252_ctx*>(v); }
void* P(uint64_t v) { return reinterpret_cast<void*>(v); }
const uint64_t* T(uint64_t v) { return reinterpret_cast<const uint64_t*>(v); }

const uint64_t MAXZ = SIZE_MAX;
const std::vector<uint64_t> COMMON = {MAXZ, 1ull << 32, (1ull << 32) - 1, 0x80000000ull, 0x7fffffffull};

std::string hex(uint64_t v) {
    char b[32];
    std::snprintf(b, sizeof b, v < 10 ? "%llu" : "0x%llx", (unsigned long long)v);
    return b;
}

void row(const Entry& e, const std::string& what, const std::vector<uint64_t>& v) {
    g_ctx->err.clear();
    const int rc = e.call(v.data());
    std::string msg = p252_last_error(e.ctx_array ? g_ctx : C(v[0]));
    for (char& c : msg)
        if (c == '\t' || c == '\n') c = ' ';
    std::printf("%s\t%s\t%d\t%s\n", e.sym, what.c_str(), rc, msg.c_str());
}

void run(Entry& e) {
    std::vector<uint64_t> good;
    for (size_t i = 0; i < e.args.size(); ++i) {
        Arg& a = e.args[i];
        if (a.kind == CTX) a.good = reinterpret_cast<uint64_t>(g_ctx);
        if (a.kind == HOST && !a.good) a.good = reinterpret_cast<uint64_t>(g_tag);
        if (a.kind == P16 || a.kind == P8 || a.kind == P4 || a.kind == P1) a.good = reinterpret_cast<uint64_t>(g_buf + 64 * (i + 1));
        good.push_back(a.good);
    }
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

const Arg CTXA = {"ctx", CTX, 0, {}}, TAGA = {"tag", HOST, 0, {}};
Arg cnt(const char* name, uint64_t good, std::vector<uint64_t> edges = {}) { return {name, CNT, good, edges}; }
Arg p16(const char* name) { return {name, P16, 0, {}}; }
Arg p8(const char* name) { return {name, P8, 0, {}}; }
Arg p4(const char* name) { return {name, P4, 0, {}}; }

// limits of the library's size checks (api.cpp): forest_shape_check, the `k > SIZE_MAX / 128 / depth` family, the ragged depths
const uint64_t FOREST_MAX_DEPTH = 64;  // FOREST_RAGGED_MAX_DEPTH = FOREST_OPENINGS_MAX_DEPTH
const uint64_t TREES_MAX = MAXZ / 8 / (FOREST_MAX_DEPTH + 2);

std::vector<Combo> forest_shape_combos() {
    return {{"n_leaves=SIZE_MAX/64", {{"n_leaves", MAXZ / 64}}},
            {"n_leaves=SIZE_MAX/64+1", {{"n_leaves", MAXZ / 64 + 1}}},
            {"n_trees=SIZE_MAX/8/66", {{"n_trees", TREES_MAX}}},
            {"n_trees=SIZE_MAX/8/66+1", {{"n_trees", TREES_MAX + 1}}},
            {"n_trees*min(max_leaves,n_leaves)=SIZE_MAX/2", {{"n_leaves", 1ull << 40}, {"max_leaves", 1ull << 41}, {"n_trees", (MAXZ / 2) >> 40}}},
            {"n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2", {{"n_leaves", 1ull << 40}, {"max_leaves", 1ull << 41}, {"n_trees", ((MAXZ / 2) >> 40) + 1}}},
            {"n_trees*max_leaves>SIZE_MAX/2,max_leaves<n_leaves", {{"n_leaves", 1ull << 50}, {"max_leaves", 1ull << 40}, {"n_trees", ((MAXZ / 2) >> 40) + 1}}}};
}

std::vector<Entry> entries() {
    std::vector<Entry> es;
    for (unsigned arity : {4u, 2u}) {
        const bool a4 = arity == 4;
        {
            // the journal's bound for the control row's sizes (n_leaves 12, n_trees 3, max_leaves 5, k 7): 7 + min(7, 12 / A^l + 3) per level
            const uint64_t jbound = a4 ? 7 + 6 + 3 : 7 + 7 + 6 + 4;
            std::vector<Combo> cs = forest_shape_combos();
            cs.push_back({"k=SIZE_MAX/128", {{"k", MAXZ / 128}}});
            cs.push_back({"k=SIZE_MAX/128+1", {{"k", MAXZ / 128 + 1}}});
            cs.push_back({"max_leaves=1,d_levels=NULL", {{"max_leaves", 1}, {"d_levels", 0}}});
            cs.push_back({"max_leaves=1,journal_cap=7", {{"max_leaves", 1}, {"journal_cap", 7}}});
            cs.push_back({"max_leaves=1,journal_cap=6", {{"max_leaves", 1}, {"journal_cap", 6}}});
            cs.push_back({"n_leaves=0,k=0", {{"n_leaves", 0}, {"k", 0}}});
            cs.push_back({"k=0,journal_cap=0,d_journal_ids=d_journal_values=NULL", {{"k", 0}, {"journal_cap", 0}, {"d_journal_ids", 0}, {"d_journal_values", 0}}});
            cs.push_back({"k=0,d_journal_len=NULL", {{"k", 0}, {"d_journal_len", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_update_journaled_device_into" : "p252_merkle2_forest_ragged_update_journaled_device_into",
                          {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p4("d_tree_ids"),
                           p8("d_leaf_ids"), p16("d_new_leaves"), cnt("k", 7), p16("d_roots"), p4("d_n_bad"), p8("d_n_hashed"), p16("d_journal_ids"),
                           p16("d_journal_values"), cnt("journal_cap", 40, {jbound - 1, jbound, MAXZ / 64, MAXZ / 64 + 1}), p8("d_journal_len")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_update_journaled_device_into : p252_merkle2_forest_ragged_update_journaled_device_into)(
                                  C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), v[5], v[6], P(v[7]), P(v[8]), P(v[9]), P(v[10]), v[11], P(v[12]), P(v[13]), P(v[14]), P(v[15]),
                                  P(v[16]), v[17], P(v[18]), nullptr);
                          },
                          cs});
            std::vector<Combo> ss = forest_shape_combos();
            ss.push_back({"max_leaves=1,d_levels=NULL", {{"max_leaves", 1}, {"d_levels", 0}}});
            ss.push_back({"n_leaves=1,d_levels=NULL", {{"n_leaves", 1}, {"d_levels", 0}}});
            ss.push_back({"journal_cap=0,every buffer NULL", {{"journal_cap", 0}, {"d_leaves", 0}, {"d_offsets", 0}, {"d_levels", 0}, {"d_journal_ids", 0},
                                                              {"d_journal_values", 0}, {"d_journal_len", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_journal_swap_device_into" : "p252_merkle2_forest_ragged_journal_swap_device_into",
                          {CTXA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p16("d_journal_ids"),
                           p16("d_journal_values"), cnt("journal_cap", 40, {MAXZ / 64, MAXZ / 64 + 1}), p8("d_journal_len"), p16("d_roots"), p4("d_n_bad")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_journal_swap_device_into : p252_merkle2_forest_ragged_journal_swap_device_into)(
                                  C(v[0]), P(v[1]), v[2], P(v[3]), v[4], v[5], P(v[6]), P(v[7]), P(v[8]), v[9], P(v[10]), P(v[11]), P(v[12]), nullptr);
                          },
                          ss});
        }
    }
    return es;
}

}  // namespace

int main() {
    g_ctx = new p252_ctx();  // device = -1: never bound
    for (Entry& e : entries()) run(e);
    delete g_ctx;
    return 0;
}
