// host_refusal_table.cpp — the argument refusals of the HOST-buffer entry points (csrc/host_io.cpp) and of the three context calls of
// csrc/api.cpp that refuse arguments (p252_scratch_residue, p252_tables_export, p252_tables_import), as a table in the format of
// api_refusals.cpp:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// (tests/test_host_refusals_cpu.py compares the lines with tests/golden/host_refusals.txt).  As there, one context that never saw a
// device reaches every check made before hipSetDevice.  Unlike the `_device` calls these READ some of their arguments while they
// check them — the offsets of the ragged calls, the positions of the openings — so those arrays are real, and the count that bounds
// the read is varied only to 0.  What lies behind hipSetDevice (the depth limit of p252_merkle4_path_batch) is not reachable here.
#include "refusal_table.hpp"

using namespace refusal;

namespace {

// three messages / trees of 2, 3 and 1 scalars, and the same with one mistake each
const uint64_t OFFSETS[4] = {0, 2, 5, 6}, DECREASING[4] = {0, 2, 1, 6}, WITH_EMPTY[4] = {0, 2, 2, 6}, TOO_LONG[2] = {0, 1ull << 59};
uint8_t POSITIONS[21], POSITION_4[21];  // n = 7 openings of depth 3; POSITION_4 holds one byte outside 0..3
unsigned char TABLE[1 << 20];           // zeros, p252_tables_size() bytes of it: never the library's table

uint64_t at(const void* p) { return reinterpret_cast<uint64_t>(p); }
Arg host(const char* name, const void* p = nullptr) { return {name, HOST, at(p), {}}; }
Arg sel(const char* name, uint64_t good, std::vector<uint64_t> edges) { return {name, INT, good, edges}; }
const uint64_t* U(uint64_t v) { return reinterpret_cast<const uint64_t*>(v); }
uint64_t* W(uint64_t v) { return reinterpret_cast<uint64_t*>(v); }

// what every call with offsets refuses of them (`count`: the name of the call's number of messages or trees); with a max_len, also
// a message longer than it, and the one message of 2^59 scalars under a max_len of `wide`
std::vector<Combo> offsets_combos(const char* count, uint64_t wide = 0) {
    std::vector<Combo> cs = {{"offsets decrease", {{"offsets", at(DECREASING)}}},
                             {"an empty message or tree", {{"offsets", at(WITH_EMPTY)}}},
                             {"one of 2^59 scalars", {{"offsets", at(TOO_LONG)}, {count, 1}}}};
    if (wide) {
        cs.back().set.push_back({"max_len", wide});
        cs.push_back({"a message longer than max_len", {{"max_len", 2}}});
    }
    return cs;
}

std::vector<Entry> entries() {
    std::vector<Entry> es;
    es.push_back({"p252_permute_batch", {CTXA, host("states"), host("out"), cnt("n", 3)},
                  [](V v) { return p252_permute_batch(C(v[0]), U(v[1]), W(v[2]), v[3]); }, {}});
    for (int trunc = 0; trunc < 2; ++trunc) {
        es.push_back({trunc ? "p252_hash_batch_truncated" : "p252_hash_batch",
                      {CTXA, TAGA, host("in"), cnt("in_len", 4), cnt("out_len", 1), host("out"), cnt("n", 3)},
                      [trunc](V v) { return (trunc ? p252_hash_batch_truncated : p252_hash_batch)(C(v[0]), T(v[1]), U(v[2]), v[3], v[4], W(v[5]), v[6]); },
                      {{"in_len=0,n=0", {{"in_len", 0}, {"n", 0}}}, {"in_len=0x80000000,n=0", {{"in_len", 0x80000000ull}, {"n", 0}}}}});
        es.push_back({trunc ? "p252_hash_ragged_truncated" : "p252_hash_ragged",
                      {CTXA, host("tags"), cnt("max_len", 40), host("in"), host("offsets", OFFSETS), cnt("out_len", 1), host("out"), sel("n", 3, {0})},
                      [trunc](V v) {
                          return (trunc ? p252_hash_ragged_truncated : p252_hash_ragged)(C(v[0]), U(v[1]), v[2], U(v[3]), U(v[4]), v[5], W(v[6]), v[7]);
                      },
                      [] {
                          std::vector<Combo> cs = offsets_combos("n", 1ull << 60);
                          cs.push_back({"out_len=0,n=0", {{"out_len", 0}, {"n", 0}}});
                          cs.push_back({"max_len=0,n=0", {{"max_len", 0}, {"n", 0}}});
                          return cs;
                      }()});
    }
    for (unsigned arity : {4u, 2u}) {
        const bool a4 = arity == 4;
        es.push_back({a4 ? "p252_merkle4_tree" : "p252_merkle2_tree", {CTXA, TAGA, host("leaves"), cnt("n_leaves", 5, {1}), host("root"), host("levels")},
                      [a4](V v) { return (a4 ? p252_merkle4_tree : p252_merkle2_tree)(C(v[0]), T(v[1]), U(v[2]), v[3], W(v[4]), W(v[5])); }, {}});
        es.push_back({a4 ? "p252_merkle4_forest_ragged" : "p252_merkle2_forest_ragged",
                      {CTXA, TAGA, host("leaves"), host("offsets", OFFSETS), sel("n_trees", 3, {0}), host("roots"), host("levels")},
                      [a4](V v) { return (a4 ? p252_merkle4_forest_ragged : p252_merkle2_forest_ragged)(C(v[0]), T(v[1]), U(v[2]), U(v[3]), v[4], W(v[5]), W(v[6])); },
                      offsets_combos("n_trees")});
    }
    es.push_back({"p252_merkle4_forest",
                  {CTXA, TAGA, host("leaves"), cnt("n_trees", 3), cnt("leaves_per_tree", 16, {1, 2, 3, 4, 8, 1ull << 62, 1ull << 63}), host("roots")},
                  [](V v) { return p252_merkle4_forest(C(v[0]), T(v[1]), U(v[2]), v[3], v[4], W(v[5])); },
                  {{"n_trees*leaves_per_tree=SIZE_MAX/32", {{"n_trees", MAXZ / 32 / 16}}},
                   {"n_trees*leaves_per_tree>SIZE_MAX/32", {{"n_trees", MAXZ / 32 / 16 + 1}}},
                   {"leaves_per_tree=3,n_trees=0", {{"leaves_per_tree", 3}, {"n_trees", 0}}}}});
    es.push_back({"p252_merkle4_path_batch",
                  {CTXA, TAGA, host("leaves"), host("siblings"), host("positions", POSITIONS), sel("depth", 3, {0}), host("roots"), sel("n", 7, {0})},
                  [](V v) {
                      return p252_merkle4_path_batch(C(v[0]), T(v[1]), U(v[2]), U(v[3]), reinterpret_cast<const uint8_t*>(v[4]), v[5], W(v[6]), v[7]);
                  },
                  {{"a position of 4", {{"positions", at(POSITION_4)}}},
                   {"depth=0,siblings=positions=NULL", {{"depth", 0}, {"siblings", 0}, {"positions", 0}}}}});
    for (int dec = 0; dec < 2; ++dec) {
        std::vector<Arg> args = {CTXA, sel("variant", 0, {1, 2, 99, (uint64_t)-1}), TAGA, host("in"), host("secrets"), host("nonces"),
                                 cnt("len", 5, {0x1fffffefull, 0x1ffffff0ull}), host("out")};
        if (dec) args.push_back(host("ok"));
        args.push_back(cnt("n", 3));
        es.push_back({dec ? "p252_decrypt_batch" : "p252_encrypt_batch", args,
                      [dec](V v) {
                          return dec ? p252_decrypt_batch(C(v[0]), (int)v[1], T(v[2]), U(v[3]), U(v[4]), U(v[5]), v[6], W(v[7]), reinterpret_cast<uint8_t*>(v[8]), v[9])
                                     : p252_encrypt_batch(C(v[0]), (int)v[1], T(v[2]), U(v[3]), U(v[4]), U(v[5]), v[6], W(v[7]), v[8]);
                      },
                      {{"variant=99,n=0", {{"variant", 99}, {"n", 0}}}, {"len=0,n=0", {{"len", 0}, {"n", 0}}}, {"len=0x1ffffff0,n=0", {{"len", 0x1ffffff0ull}, {"n", 0}}}}});
        args = {CTXA, sel("variant", 0, {1, 2, 99, (uint64_t)-1}), host("tags"), cnt("max_len", 40, {2048, 2049}), host("in"), host("offsets", OFFSETS),
                host("secrets"), host("nonces"), host("out")};
        if (dec) args.push_back(host("ok"));
        args.push_back(sel("n", 3, {0}));
        std::vector<Combo> cs = offsets_combos("n", 2048);
        cs.push_back({"variant=99,n=0", {{"variant", 99}, {"n", 0}}});
        cs.push_back({"max_len=0,n=0", {{"max_len", 0}, {"n", 0}}});
        es.push_back({dec ? "p252_decrypt_ragged" : "p252_encrypt_ragged", args,
                      [dec](V v) {
                          return dec ? p252_decrypt_ragged(C(v[0]), (int)v[1], U(v[2]), v[3], U(v[4]), U(v[5]), U(v[6]), U(v[7]), W(v[8]), reinterpret_cast<uint8_t*>(v[9]),
                                                           v[10])
                                     : p252_encrypt_ragged(C(v[0]), (int)v[1], U(v[2]), v[3], U(v[4]), U(v[5]), U(v[6]), U(v[7]), W(v[8]), v[9]);
                      },
                      cs});
    }
    es.push_back({"p252_scratch_residue", {CTXA, host("nonzero_bytes", TABLE)}, [](V v) { return p252_scratch_residue(C(v[0]), W(v[1])); }, {}});
    const uint64_t len = p252_tables_size();
    es.push_back({"p252_tables_export", {CTXA, host("host_buf", TABLE), sel("len", len, {0, len - 1, len + 1})},
                  [](V v) { return p252_tables_export(C(v[0]), P(v[1]), v[2]); }, {}});
    // (its control row is a refusal too: the one table it accepts comes out of a device)
    es.push_back({"p252_tables_import", {CTXA, host("host_buf", TABLE), sel("len", len, {0, len - 1, len + 1})},
                  [](V v) { return p252_tables_import(C(v[0]), P(v[1]), v[2]); }, {}});
    return es;
}

}  // namespace

int main() {
    if (p252_tables_size() > sizeof TABLE) return 2;
    POSITION_4[5] = 4;
    g_ctx = new p252_ctx();  // device = -1: never bound
    for (Entry& e : entries()) run(e);
    delete g_ctx;
    return 0;
}
