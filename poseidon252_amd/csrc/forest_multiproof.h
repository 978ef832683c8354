// forest_multiproof.h — launch interface between api_forest.cpp and forest_multiproof.hip: k (tree id, leaf id) pairs anywhere in a built
// forest of trees of DIFFERENT sizes proved by one shared, tree-major proof (p252_merkle{4,2}_forest_ragged_multiproof_device_into: data
// movement only) and checked with every ancestor hashed once (p252_merkle{4,2}_forest_ragged_multiproof_verify_device_into).  Each
// tree's part of the proof is the single-tree proof of multiproof.h; the format is in include/poseidon252_hip.h and DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_MULTIPROOF_MAX_DEPTH = 32;  // max_leaves < 2^32: a node index fits in a record word

// The host's view of one call, all derived from (arity, n_leaves, n_trees, max_leaves, k).  in[l] = the most elements of S_l over all
// trees together: min(k, n_leaves / arity^l + n_trees) (ForestRaggedPlan's bound of a level) — what the launches of level l are sized
// by; the true counts stay on the device.
struct ForestMultiproofPlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    size_t k = 0, n_trees = 0, n_leaves = 0, max_leaves = 0;
    size_t in[FOREST_MULTIPROOF_MAX_DEPTH + 2] = {};
    size_t tiles = 0, tree_tiles = 0;  // scan tiles of the pairs (256 elements) and of the trees (2,048 trees)
    size_t bound = 0;                  // p252_merkle{4,2}_forest_ragged_multiproof_bound
    size_t index_bytes = 0;            // the forest's index (launch_forest_ragged_index)
    size_t tree_bytes = 0;             // per tree: the counters of one call, 60 bytes a tree and 8 per 2,048 trees, plus 1 KiB
    size_t pair_bytes = 0;             // per pair: S_0 (nodes and trees), two tree lists, two record lists, the widths: 52 bytes a pair
                                       // and 20 per 256 pairs
    size_t work_bytes() const { return index_bytes + tree_bytes + pair_bytes; }
    size_t values_bytes() const { return 2 * k * 32; }  // verify only: two lists of node values, 64 bytes a pair
};
ForestMultiproofPlan forest_multiproof_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);

// Extraction on `st`: work = plan.work_bytes() of scratch.  proof may be null when proof_cap == 0; n_bad (uint32) may be null.
hipError_t launch_forest_multiproof(const ForestMultiproofPlan& plan, const void* leaves, const void* offsets, const void* levels,
                                    const void* tree_ids, const void* leaf_ids, void* leaves_out, void* proof, size_t proof_cap,
                                    void* proof_offsets, void* n_bad, void* work, hipStream_t st);

// Verification on `st`: work = plan.work_bytes(), values = plan.values_bytes() of scratch.  proof may be null when proof_len == 0;
// roots_out, n_hashed (uint64) and n_bad (uint32) may be null.
hipError_t launch_forest_multiproof_verify(const int32_t* tab, const TagArg& tag, const ForestMultiproofPlan& plan, const void* offsets,
                                           const void* tree_ids, const void* leaf_ids, const void* leaves_in, const void* proof,
                                           size_t proof_len, const void* proof_offsets, const void* roots, void* ok, void* roots_out,
                                           void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st);

}  // namespace p252
