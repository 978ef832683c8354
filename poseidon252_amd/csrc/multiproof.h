// multiproof.h — launch interface between api.cpp and multiproof.hip: k leaves of ONE stored tree proved by one shared proof
// (p252_merkle{4,2}_multiproof_device: data movement only) and checked with every ancestor hashed once
// (p252_merkle{4,2}_multiproof_verify_device).  The proof format is in include/poseidon252_hip.h and DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned MULTIPROOF_MAX_DEPTH = 32;  // an arity-2 tree of 2^32 - 1 leaves (positions are uint32)

// The host's view of one call, all derived from (arity, n_leaves, k).  w[l] = nodes of level l (w[0] = n_leaves, w[depth] = 1),
// start[l] = where level l >= 1 begins inside d_levels, in[l] = min(k, w[l]) = the most nodes of S_l: what the launches of level l
// are sized by (the true counts stay on the device).
struct MultiproofPlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    size_t k = 0;
    size_t w[MULTIPROOF_MAX_DEPTH + 1] = {};
    size_t start[MULTIPROOF_MAX_DEPTH + 1] = {};
    size_t in[MULTIPROOF_MAX_DEPTH + 1] = {};
    size_t tiles = 0;  // scan tiles of the widest level (level 0)
    size_t bound = 0;  // p252_merkle{4,2}_multiproof_bound(n_leaves, k)
    size_t count_bytes = 0, tile_bytes = 0, list_bytes = 0, value_bytes = 0;
    size_t work_bytes() const { return count_bytes + tile_bytes + 2 * list_bytes; }  // counters, scan tiles, two work lists
    size_t values_bytes() const { return 2 * value_bytes; }                          // verify only: two lists of node values
};
MultiproofPlan multiproof_plan(unsigned arity, size_t n_leaves, size_t k);

// Extraction on `st`: work = plan.work_bytes() of scratch.  proof may be null when proof_cap == 0; n_bad (uint32) may be null.
hipError_t launch_multiproof(const MultiproofPlan& plan, const void* leaves, const void* levels, const void* indices, void* leaves_out,
                             void* proof, size_t proof_cap, void* proof_len, void* n_bad, void* work, hipStream_t st);

// Verification on `st`: work = plan.work_bytes(), values = plan.values_bytes() of scratch.  proof may be null when proof_len == 0;
// root_out, n_hashed (uint64) and n_bad (uint32) may be null.
hipError_t launch_multiproof_verify(const int32_t* tab, const TagArg& tag, const MultiproofPlan& plan, const void* indices,
                                    const void* leaves_in, const void* proof, size_t proof_len, const void* root, void* ok, void* root_out,
                                    void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st);

// One level's digests over a record list that the CALLER made (forest_multiproof.hip), by the kernels of the verification above.
// Record g < *count (16 bytes): parent index, start of its run in vals_in, proof offset bits 0 .. 59 with the mask of the child
// slots that vals_in holds above them.  Child slot j of record g exists while parent * arity + j < w_node[g]; it comes from vals_in,
// from proof (zero at or past proof_len) or is zero; the digest goes to vals_out[g].  bound = the host's bound of *count.
struct MultiproofDigestList {
    const void* list = nullptr;
    const unsigned long long* count = nullptr;
    const void* vals_in = nullptr;
    void* vals_out = nullptr;
    const void* proof = nullptr;
    size_t proof_len = 0;
    const uint32_t* w_node = nullptr;
    size_t bound = 0;
};
hipError_t launch_multiproof_digest_list(const int32_t* tab, const TagArg& tag, unsigned arity, const MultiproofDigestList& list,
                                         hipStream_t st);

}  // namespace p252
