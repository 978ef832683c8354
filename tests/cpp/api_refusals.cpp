// api_refusals.cpp — the argument refusals of every `_device` entry point of libposeidon252_hip.so, as a table.
//
// Every refusal happens before the entry point binds its device, so ONE context that never saw a device (device = -1) reaches all
// of them on a machine with or without a GPU.  For each entry point the program starts from an all-good argument set — the control
// row, which must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP — and varies one argument at a time:
// ctx NULL, every pointer NULL, every aligned array off by half its alignment, every count at 0 and at both sides of every size
// check of the library.  One line per case:   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// (tests/test_api_refusals_cpu.py compares the lines with tests/golden/api_refusals.txt).  No pointer is dereferenced: no case
// reaches a device.
// `api_refusals --pairs` prints other rows instead, which no file records: two arguments varied at once, for every pair of arguments of
// every entry point (refusal_table.hpp run_pairs) — what a change that must keep the order of the checks is compared on, old library
// against new.
#include <cstring>

#include "refusal_table.hpp"

using namespace refusal;

namespace {

std::vector<Entry> entries() {
    std::vector<Entry> es;
    es.push_back({"p252_permute_batch_device", {CTXA, p16("d_states"), p16("d_out"), cnt("n", 3)},
                  [](V v) { return p252_permute_batch_device(C(v[0]), P(v[1]), P(v[2]), v[3], nullptr); }, {}});
    for (int trunc = 0; trunc < 2; ++trunc) {
        es.push_back({trunc ? "p252_hash_batch_truncated_device" : "p252_hash_batch_device",
                      {CTXA, TAGA, p16("d_in"), cnt("in_len", 4), cnt("out_len", 1), p16("d_out"), cnt("n", 3)},
                      [trunc](V v) {
                          return (trunc ? p252_hash_batch_truncated_device : p252_hash_batch_device)(C(v[0]), T(v[1]), P(v[2]), v[3], v[4], P(v[5]), v[6], nullptr);
                      },
                      {{"in_len=0,n=0", {{"in_len", 0}, {"n", 0}}}, {"in_len=2", {{"in_len", 2}}}, {"in_len=42,out_len=5", {{"in_len", 42}, {"out_len", 5}}}}});
        es.push_back({trunc ? "p252_hash_ragged_truncated_device" : "p252_hash_ragged_device",
                      {CTXA, p16("d_tags"), cnt("max_len", 40), p16("d_in"), p8("d_offsets"), cnt("out_len", 1), p16("d_out"),
                       cnt("n", 3, {MAXZ / 64 - 1, MAXZ / 64}), p4("d_n_bad")},
                      [trunc](V v) {
                          return (trunc ? p252_hash_ragged_truncated_device : p252_hash_ragged_device)(C(v[0]), P(v[1]), v[2], P(v[3]), P(v[4]), v[5], P(v[6]), v[7],
                                                                                                       P(v[8]), nullptr);
                      },
                      {{"out_len=16,n=SIZE_MAX/128-1", {{"out_len", 16}, {"n", MAXZ / 128 - 1}}},
                       {"out_len=16,n=SIZE_MAX/128", {{"out_len", 16}, {"n", MAXZ / 128}}},
                       {"out_len=0,n=0", {{"out_len", 0}, {"n", 0}}},
                       {"max_len=0,n=0", {{"max_len", 0}, {"n", 0}}}}});
    }
    for (unsigned arity : {4u, 2u}) {
        const bool a4 = arity == 4;
        const uint64_t fdepth = a4 ? 2 : 3;  // levels above a tree of max_leaves = 5
        es.push_back({a4 ? "p252_merkle4_tree_device" : "p252_merkle2_tree_device",
                      {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 5, {1}), p16("d_root"), p16("d_levels")},
                      [a4](V v) { return (a4 ? p252_merkle4_tree_device : p252_merkle2_tree_device)(C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), P(v[5]), nullptr); },
                      {}});
        es.push_back({a4 ? "p252_merkle4_forest_device" : "p252_merkle2_forest_device",
                      {CTXA, TAGA, p16("d_leaves"), cnt("n_trees", 3), cnt("leaves_per_tree", 16, {1, 2, 3, 4, 8, 24, 1ull << 61, 1ull << 62, 1ull << 63}), p16("d_roots"),
                       p16("d_levels")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_forest_device : p252_merkle2_forest_device)(C(v[0]), T(v[1]), P(v[2]), v[3], v[4], P(v[5]), P(v[6]), nullptr);
                      },
                      {{"n_trees*leaves_per_tree=SIZE_MAX/32", {{"n_trees", MAXZ / 32 / 16}}},
                       {"n_trees*leaves_per_tree>SIZE_MAX/32", {{"n_trees", MAXZ / 32 / 16 + 1}}},
                       {"leaves_per_tree=3,n_trees=0", {{"leaves_per_tree", 3}, {"n_trees", 0}}}}});
        es.push_back({a4 ? "p252_merkle4_forest_ragged_device" : "p252_merkle2_forest_ragged_device",
                      {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_roots"), p16("d_levels"),
                       p4("d_n_bad")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_forest_ragged_device : p252_merkle2_forest_ragged_device)(C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), v[5], v[6], P(v[7]),
                                                                                                              P(v[8]), P(v[9]), nullptr);
                      },
                      forest_shape_combos()});
        {
            std::vector<Combo> cs = forest_shape_combos();
            cs.push_back({"k=SIZE_MAX/128/depth", {{"k", MAXZ / 128 / fdepth}}});
            cs.push_back({"k=SIZE_MAX/128/depth+1", {{"k", MAXZ / 128 / fdepth + 1}}});
            cs.push_back({"max_leaves=1,k=SIZE_MAX/128", {{"max_leaves", 1}, {"k", MAXZ / 128}}});
            cs.push_back({"max_leaves=1,k=SIZE_MAX/128+1", {{"max_leaves", 1}, {"k", MAXZ / 128 + 1}}});
            cs.push_back({"max_leaves=1,d_levels=d_siblings=d_positions=NULL", {{"max_leaves", 1}, {"d_levels", 0}, {"d_siblings", 0}, {"d_positions", 0}}});
            cs.push_back({"n_leaves=0,k=0", {{"n_leaves", 0}, {"k", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_openings_device" : "p252_merkle2_forest_ragged_openings_device",
                          {CTXA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p4("d_tree_ids"),
                           p8("d_leaf_ids"), cnt("k", 7), p16("d_leaves_out"), p16("d_siblings"), p1("d_positions"), p1("d_depths"), p4("d_n_bad")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_openings_device : p252_merkle2_forest_ragged_openings_device)(
                                  C(v[0]), P(v[1]), v[2], P(v[3]), v[4], v[5], P(v[6]), P(v[7]), P(v[8]), v[9], P(v[10]), P(v[11]), P(v[12]), P(v[13]), P(v[14]), nullptr);
                          },
                          cs});
        }
        const std::vector<Combo> stride_combos = {{"k=SIZE_MAX/128/stride_depth", {{"k", MAXZ / 128 / 3}}},
                                                  {"k=SIZE_MAX/128/stride_depth+1", {{"k", MAXZ / 128 / 3 + 1}}},
                                                  {"stride_depth=0,k=SIZE_MAX/128", {{"stride_depth", 0}, {"k", MAXZ / 128}}},
                                                  {"stride_depth=0,k=SIZE_MAX/128+1", {{"stride_depth", 0}, {"k", MAXZ / 128 + 1}}},
                                                  {"stride_depth=0,d_siblings=d_positions=NULL", {{"stride_depth", 0}, {"d_siblings", 0}, {"d_positions", 0}}},
                                                  {"stride_depth=0,d_siblings+8", {{"stride_depth", 0}, {"d_siblings", reinterpret_cast<uint64_t>(g_buf + 64 * 4 + 8)}}},
                                                  {"stride_depth=65,k=0", {{"stride_depth", 65}, {"k", 0}}}};
        es.push_back({a4 ? "p252_merkle4_path_ragged_device" : "p252_merkle2_path_ragged_device",
                      {CTXA, TAGA, p16("d_leaves_in"), p16("d_siblings"), p1("d_positions"), p1("d_depths"), cnt("stride_depth", 3, {64, 65}), p16("d_roots_out"),
                       cnt("k", 7), p4("d_n_bad")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_path_ragged_device : p252_merkle2_path_ragged_device)(C(v[0]), T(v[1]), P(v[2]), P(v[3]), P(v[4]), P(v[5]), v[6], P(v[7]),
                                                                                                          v[8], P(v[9]), nullptr);
                      },
                      stride_combos});
        {
            std::vector<Combo> cs = stride_combos;
            cs.push_back({"n_trees=0,d_roots=NULL", {{"n_trees", 0}, {"d_roots", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_verify_device" : "p252_merkle2_forest_ragged_verify_device",
                          {CTXA, TAGA, p16("d_leaves_in"), p16("d_siblings"), p1("d_positions"), p1("d_depths"), cnt("stride_depth", 3, {64, 65}), p4("d_tree_ids"),
                           p16("d_roots"), cnt("n_trees", 3), p1("d_ok"), cnt("k", 7)},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_verify_device : p252_merkle2_forest_ragged_verify_device)(
                                  C(v[0]), T(v[1]), P(v[2]), P(v[3]), P(v[4]), P(v[5]), v[6], P(v[7]), P(v[8]), v[9], P(v[10]), v[11], nullptr);
                          },
                          cs});
        }
        {
            std::vector<Combo> cs = forest_shape_combos();
            cs.push_back({"k=SIZE_MAX/128", {{"k", MAXZ / 128}}});
            cs.push_back({"k=SIZE_MAX/128+1", {{"k", MAXZ / 128 + 1}}});
            cs.push_back({"max_leaves=1,d_levels=NULL", {{"max_leaves", 1}, {"d_levels", 0}}});
            cs.push_back({"n_leaves=1,d_levels=NULL", {{"n_leaves", 1}, {"d_levels", 0}}});
            cs.push_back({"n_leaves=0,k=0", {{"n_leaves", 0}, {"k", 0}}});
            es.push_back({a4 ? "p252_merkle4_forest_ragged_update_device" : "p252_merkle2_forest_ragged_update_device",
                          {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 12), p8("d_offsets"), cnt("n_trees", 3), cnt("max_leaves", 5), p16("d_levels"), p4("d_tree_ids"),
                           p8("d_leaf_ids"), p16("d_new_leaves"), cnt("k", 7), p16("d_roots"), p4("d_n_bad"), p8("d_n_hashed")},
                          [a4](V v) {
                              return (a4 ? p252_merkle4_forest_ragged_update_device : p252_merkle2_forest_ragged_update_device)(
                                  C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), v[5], v[6], P(v[7]), P(v[8]), P(v[9]), P(v[10]), v[11], P(v[12]), P(v[13]), P(v[14]), nullptr);
                          },
                          cs});
        }
        const std::vector<Combo> depth_combos = {{"depth=0,d_siblings=d_positions=NULL", {{"depth", 0}, {"d_siblings", 0}, {"d_positions", 0}}},
                                                 {"depth=0,d_siblings+8", {{"depth", 0}, {"d_siblings", reinterpret_cast<uint64_t>(g_buf + 64 * 4 + 8)}}},
                                                 {"depth=0x10000,n=0", {{"depth", 0x10000}, {"n", 0}}}};
        es.push_back({a4 ? "p252_merkle4_path_batch_device" : "p252_merkle2_path_batch_device",
                      {CTXA, TAGA, p16("d_leaves"), p16("d_siblings"), p1("d_positions"), cnt("depth", 3, {0xffff, 0x10000}), p16("d_roots"), cnt("n", 7)},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_path_batch_device : p252_merkle2_path_batch_device)(C(v[0]), T(v[1]), P(v[2]), P(v[3]), P(v[4]), v[5], P(v[6]), v[7], nullptr);
                      },
                      depth_combos});
        es.push_back({a4 ? "p252_merkle4_verify_batch_device" : "p252_merkle2_verify_batch_device",
                      {CTXA, TAGA, p16("d_leaves"), p16("d_siblings"), p1("d_positions"), cnt("depth", 3, {0xffff, 0x10000}), p16("d_root"), p1("d_ok"),
                       cnt("n", 7, {MAXZ / 32, MAXZ / 32 + 1})},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_verify_batch_device : p252_merkle2_verify_batch_device)(C(v[0]), T(v[1]), P(v[2]), P(v[3]), P(v[4]), v[5], P(v[6]), P(v[7]),
                                                                                                            v[8], nullptr);
                      },
                      depth_combos});
        es.push_back({a4 ? "p252_merkle4_openings_device" : "p252_merkle2_openings_device",
                      {CTXA, p16("d_leaves"), cnt("n_leaves", 10, {1}), p16("d_levels"), p4("d_indices"), cnt("k", 7), p16("d_leaves_out"), p16("d_siblings"),
                       p1("d_positions"), p4("d_n_bad")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_openings_device : p252_merkle2_openings_device)(C(v[0]), P(v[1]), v[2], P(v[3]), P(v[4]), v[5], P(v[6]), P(v[7]), P(v[8]),
                                                                                                    P(v[9]), nullptr);
                      },
                      {{"n_leaves=1,d_levels=d_siblings=d_positions=NULL", {{"n_leaves", 1}, {"d_levels", 0}, {"d_siblings", 0}, {"d_positions", 0}}},
                       {"n_leaves=0,k=0", {{"n_leaves", 0}, {"k", 0}}}}});
        es.push_back({a4 ? "p252_merkle4_multiproof_device" : "p252_merkle2_multiproof_device",
                      {CTXA, p16("d_leaves"), cnt("n_leaves", 10, {1}), p16("d_levels"), p4("d_indices"), cnt("k", 7), p16("d_leaves_out"), p16("d_proof"),
                       cnt("proof_cap", 20), p8("d_proof_len"), p4("d_n_bad")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_multiproof_device : p252_merkle2_multiproof_device)(C(v[0]), P(v[1]), v[2], P(v[3]), P(v[4]), v[5], P(v[6]), P(v[7]), v[8],
                                                                                                        P(v[9]), P(v[10]), nullptr);
                      },
                      {{"proof_cap=0,d_proof=NULL", {{"proof_cap", 0}, {"d_proof", 0}}},
                       {"n_leaves=1,d_levels=NULL", {{"n_leaves", 1}, {"d_levels", 0}}},
                       {"n_leaves=k=0xffffffff", {{"n_leaves", 0xffffffffull}, {"k", 0xffffffffull}}}}});
        es.push_back({a4 ? "p252_merkle4_multiproof_verify_device" : "p252_merkle2_multiproof_verify_device",
                      {CTXA, TAGA, cnt("n_leaves", 10, {1}), p4("d_indices"), p16("d_leaves_in"), cnt("k", 7), p16("d_proof"), cnt("proof_len", 9, {MAXZ / 32, MAXZ / 32 + 1}),
                       p16("d_root"), p1("d_ok"), p16("d_root_out"), p8("d_n_hashed"), p4("d_n_bad")},
                      [a4](V v) {
                          return (a4 ? p252_merkle4_multiproof_verify_device : p252_merkle2_multiproof_verify_device)(
                              C(v[0]), T(v[1]), v[2], P(v[3]), P(v[4]), v[5], P(v[6]), v[7], P(v[8]), P(v[9]), P(v[10]), P(v[11]), P(v[12]), nullptr);
                      },
                      {{"proof_len=0,d_proof=NULL", {{"proof_len", 0}, {"d_proof", 0}}},
                       {"n_leaves=k=0xffffffff", {{"n_leaves", 0xffffffffull}, {"k", 0xffffffffull}}}}});
    }
    for (int checked = 0; checked < 2; ++checked) {
        std::vector<Arg> args = {CTXA, TAGA, p16("d_leaves"), cnt("n_leaves", 10, {1}), p16("d_levels"), p4("d_indices"), p16("d_new_leaves"), cnt("k", 3), p16("d_root")};
        if (checked) args.push_back(p4("d_n_bad"));
        es.push_back({checked ? "p252_merkle4_update_checked_device" : "p252_merkle4_update_device", args,
                      [checked](V v) {
                          return checked ? p252_merkle4_update_checked_device(C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), P(v[5]), P(v[6]), v[7], P(v[8]), P(v[9]), nullptr)
                                         : p252_merkle4_update_device(C(v[0]), T(v[1]), P(v[2]), v[3], P(v[4]), P(v[5]), P(v[6]), v[7], P(v[8]), nullptr);
                      },
                      {{"k=0,d_indices=d_new_leaves=NULL", {{"k", 0}, {"d_indices", 0}, {"d_new_leaves", 0}}}, {"n_leaves=1,d_levels=NULL", {{"n_leaves", 1}, {"d_levels", 0}}}}});
    }
    es.push_back({"p252_truncate250_device", {CTXA, p16("d_scalars"), p16("d_out_raw"), cnt("n", 3)},
                  [](V v) { return p252_truncate250_device(C(v[0]), P(v[1]), P(v[2]), v[3], nullptr); }, {}});
    es.push_back({"p252_to_bytes_device", {CTXA, p16("d_scalars"), p16("d_bytes"), cnt("n", 3)},
                  [](V v) { return p252_to_bytes_device(C(v[0]), P(v[1]), P(v[2]), v[3], nullptr); }, {}});
    es.push_back({"p252_from_bytes_device", {CTXA, p16("d_bytes"), p16("d_scalars"), p1("d_ok"), cnt("n", 3)},
                  [](V v) { return p252_from_bytes_device(C(v[0]), P(v[1]), P(v[2]), P(v[3]), v[4], nullptr); }, {}});
    for (int dec = 0; dec < 2; ++dec) {
        std::vector<Arg> args = {CTXA, {"variant", INT, 0, {1, 2, 99, (uint64_t)-1}}, TAGA, p16("d_in"), p16("d_secrets"), p16("d_nonces"),
                                 cnt("len", 5, {0x1fffffefull, 0x1ffffff0ull}), p16("d_out")};
        if (dec) args.push_back(p1("d_ok"));
        args.push_back(cnt("n", 3));
        es.push_back({dec ? "p252_decrypt_batch_device" : "p252_encrypt_batch_device", args,
                      [dec](V v) {
                          return dec ? p252_decrypt_batch_device(C(v[0]), (int)v[1], T(v[2]), P(v[3]), P(v[4]), P(v[5]), v[6], P(v[7]), P(v[8]), v[9], nullptr)
                                     : p252_encrypt_batch_device(C(v[0]), (int)v[1], T(v[2]), P(v[3]), P(v[4]), P(v[5]), v[6], P(v[7]), v[8], nullptr);
                      },
                      {{"variant=99,n=0", {{"variant", 99}, {"n", 0}}}, {"len=0,n=0", {{"len", 0}, {"n", 0}}}}});
    }
    es.push_back({"p252_clock_probe_device", {CTXA, p8("d_out6"), {"spin_us", INT, 1000, {0, 1000000, 1000001, 0xffffffffull}}},
                  [](V v) { return p252_clock_probe_device(C(v[0]), P(v[1]), (unsigned)v[2], nullptr); }, {}});
    return es;
}

// the two multi-context entry points take an ARRAY of contexts: the one device-less context, once or twice
void multi_rows(bool pairs) {
    static p252_ctx* one[1];
    static p252_ctx* twice[2];
    static const void* d_in[1] = {g_buf + 64};
    static void* d_out[1] = {g_buf + 128};
    static size_t n_per[1] = {3};
    one[0] = twice[0] = twice[1] = g_ctx;
    auto host = [](const char* name, const void* p) { return Arg{name, HOST, reinterpret_cast<uint64_t>(p), {}}; };
    const Arg n_ctx = {"n_ctx", INT, 1, {0}};  // (more than the array holds would be read)
    const std::vector<Combo> dup = {{"ctxs=the same context twice", {{"ctxs", reinterpret_cast<uint64_t>(twice)}, {"n_ctx", 2}}}};
    std::vector<Entry> es;
    es.push_back({"p252_hash_batch_multi_device",
                  {host("ctxs", one), n_ctx, TAGA, host("d_in", d_in), cnt("in_len", 4), cnt("out_len", 1), host("d_out", d_out), host("n_per_ctx", n_per)},
                  [](V v) {
                      return p252_hash_batch_multi_device(reinterpret_cast<p252_ctx* const*>(v[0]), v[1], T(v[2]), reinterpret_cast<const void* const*>(v[3]), v[4], v[5],
                                                          reinterpret_cast<void* const*>(v[6]), reinterpret_cast<const size_t*>(v[7]), nullptr);
                  },
                  dup, true});
    es.push_back({"p252_merkle4_tree_multi_device",
                  {host("ctxs", one), n_ctx, TAGA, host("d_leaves", d_in), cnt("leaves_per_ctx", 16, {1, 2, 8, 1ull << 62, 1ull << 63}), host("root", g_buf + 192)},
                  [](V v) {
                      return p252_merkle4_tree_multi_device(reinterpret_cast<p252_ctx* const*>(v[0]), v[1], T(v[2]), reinterpret_cast<const void* const*>(v[3]), v[4],
                                                            reinterpret_cast<uint64_t*>(v[5]));
                  },
                  dup, true});
    for (Entry& e : es) pairs ? run_pairs(e) : run(e);
    if (pairs) return;
    // the sharded build takes a communicator, which only RCCL ranks can make: its one reachable refusal
    const int rc = p252_merkle4_tree_sharded_device(nullptr, g_tag, g_buf + 64, 16, g_buf + 128, nullptr);
    std::printf("p252_merkle4_tree_sharded_device\tcomm=NULL\t%d\t\n", rc);
}

}  // namespace

int main(int argc, char** argv) {
    const bool pairs = argc > 1 && !std::strcmp(argv[1], "--pairs");
    g_ctx = new p252_ctx();  // device = -1: never bound
    for (Entry& e : entries()) pairs ? run_pairs(e) : run(e);
    multi_rows(pairs);
    delete g_ctx;
    return 0;
}
