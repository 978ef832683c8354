// forest_sequential.h — launch interface between api_forest.cpp and forest_sequential.hip: k leaf updates of a built ragged forest
// applied IN ORDER in one call (p252_merkle{4,2}_forest_ragged_update_sequential_device_into): update i sees the forest as updates
// 0 .. i - 1 left it, the same (tree, leaf) pair may occur any number of times, and every update gets its witness — the old leaf, its
// opening in the state just before the update (the layout of forest_openings.h) and the tree's root before and after.  The work is
// parallel level by level over a list of the updates kept sorted by (tree, node, time): include/poseidon252_hip.h and DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_SEQUENTIAL_MAX_DEPTH = 32;  // max_leaves < 2^32: a node index is one word of a list's key

// the work area of a call with k updates, offsets into the first scratch buffer behind the forest's index: the counters, two lists of
// 16-byte keys {tree, node, time, depth of the tree} with their 32-byte values (the list of level l and the one of level l + 1), the
// parents' values as the digest launch stores them, and per element and child slot two words of the merge rank.  The second buffer
// holds one level's gathered children, k x arity scalars.  (128 + 40 arity bytes an update: 288 at arity 4, 208 at arity 2.)
struct ForestSequentialWork {
    size_t ctr, keys[2], vals[2], parents, ranks, bytes, children_bytes;
};
inline ForestSequentialWork forest_sequential_work(unsigned arity, size_t k) {
    ForestSequentialWork w{};
    w.ctr = 0;
    w.keys[0] = 256;
    w.keys[1] = w.keys[0] + k * 16;
    w.vals[0] = w.keys[1] + k * 16;
    w.vals[1] = w.vals[0] + k * 32;
    w.parents = w.vals[1] + k * 32;
    w.ranks = w.parents + k * 32;
    w.bytes = w.ranks + k * arity * 8;
    w.children_bytes = k * arity * 32;
    return w;
}

// ntree / lo = the forest's index (launch_forest_ragged_index); work / children = the two areas above; stride_depth =
// depth(max_leaves) <= FOREST_SEQUENTIAL_MAX_DEPTH; k < 2^32.  old_leaves, roots_before, roots, n_bad (uint32) and n_hashed (uint64)
// may be null; levels, siblings and positions may be null when stride_depth == 0.  The digests are launch_merkle4's, one launch of k
// nodes per level over the children that k_sq_gather laid out.
hipError_t launch_forest_update_sequential(unsigned arity, const int32_t* tab, const TagArg& tag, void* leaves, const void* offsets,
                                           const uint64_t* ntree, const uint64_t* lo, size_t n_trees, void* levels, const void* tree_ids,
                                           const void* leaf_ids, const void* new_leaves, const void* order, size_t k, unsigned stride_depth,
                                           void* old_leaves, void* siblings, void* positions, void* depths, void* roots_before,
                                           void* roots_after, void* roots, void* n_bad, void* n_hashed, void* work, void* children,
                                           hipStream_t st);

}  // namespace p252
