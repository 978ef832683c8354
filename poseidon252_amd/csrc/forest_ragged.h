// forest_ragged.h — launch interface between api.cpp and forest_ragged.hip: a forest of Merkle trees of DIFFERENT sizes in one
// call (p252_merkle{4,2}_forest_ragged*).  Tree t = leaves[offsets[t] .. offsets[t+1]); each tree is exactly what
// p252_merkle{4,2}_tree builds (levels zero-padded to a multiple of the arity, a single leaf is its own root).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_RAGGED_MAX_DEPTH = 64;

// The host's view of one call: sizes of the bookkeeping and of every level, all derived from (n_leaves, n_trees, max_leaves).
// Level l (1 .. depth) of all trees together has at most bound[l] = n_leaves / arity^l + n_trees nodes (the leaves of the good
// trees never add up to more than n_leaves: forest_ragged.hip).
struct ForestRaggedPlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    bool levels = false;  // the caller's d_levels is written (tree-major) instead of the level-major scratch
    size_t n_trees = 0, n_leaves = 0, tiles = 0;
    size_t bound[FOREST_RAGGED_MAX_DEPTH + 1] = {};
    size_t first_off[FOREST_RAGGED_MAX_DEPTH + 1] = {};  // level l's first-tree-of-block row in the bookkeeping (uint64 entries)
    size_t first_len[FOREST_RAGGED_MAX_DEPTH + 1] = {};
    size_t meta_bytes = 0;  // the bookkeeping: per-tree leaf counts, the scans, the first-tree rows (a multiple of 256 bytes)
};

// levels above the leaves of a tree of n leaves, for the plans and api.cpp's checks: p252_merkle{4,2}_depth without its wrap-around at SIZE_MAX
unsigned forest_ragged_depth(size_t n, unsigned arity);
ForestRaggedPlan forest_ragged_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, bool levels);

// The whole build on `st`: validation and scans over the trees, then one digest launch per level across all trees.  meta =
// plan.meta_bytes of scratch; lvl_a / lvl_b = the level-major ping-pong (bound[1] / bound[2] scalars; unused with plan.levels).
// n_bad (device uint32, may be null) is incremented once per bad tree, whose root is written as zero.
hipError_t launch_forest_ragged(const int32_t* tab, const TagArg& tag, const ForestRaggedPlan& plan, const void* leaves,
                                const void* offsets, size_t max_leaves, void* roots, void* levels, void* n_bad, void* meta,
                                void* lvl_a, void* lvl_b, hipStream_t st);

// The forest's index alone, for calls that READ a built forest (forest_openings.hip): the build's own validation and scans into
// `meta` (forest_ragged_index_bytes(n_trees) of scratch) — *ntree = the n_trees leaf counts (0: a bad tree), *lo = the n_trees + 1
// block starts of the tree-major levels.  No root is written and nothing is counted.
size_t forest_ragged_index_bytes(size_t n_trees);
hipError_t launch_forest_ragged_index(unsigned arity, const void* offsets, size_t n_trees, size_t n_leaves, size_t max_leaves, void* meta,
                                      const uint64_t** ntree, const uint64_t** lo, hipStream_t st);

}  // namespace p252
