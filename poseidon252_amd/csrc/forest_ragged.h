// forest_ragged.h — launch interface between api_forest.cpp and forest_ragged.hip: a forest of Merkle trees of DIFFERENT sizes in one
// call (p252_merkle{4,2}_forest_ragged*).  Tree t = leaves[offsets[t] .. offsets[t+1]); each tree is exactly what
// p252_merkle{4,2}_tree builds (levels zero-padded to a multiple of the arity, a single leaf is its own root).
// Also the select of such forests (p252_merkle{4,2}_forest_ragged_select_device_into): trees gathered into a new forest, nothing hashed.
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

// levels above the leaves of a tree of n leaves, for the plans and api_forest.cpp's checks: p252_merkle{4,2}_depth without its wrap-around at SIZE_MAX
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

// The build's three-pass scan over `rows` rows of n uint64 values each that the CALLER wrote (values[row * n + i]): in place, every value
// becomes the sum of its row's values before it, and totals[row] (device) the row's sum.  tsum = rows * forest_scan_rows_tiles(n) words
// of scratch.  Three launches whatever rows is.
size_t forest_scan_rows_tiles(size_t n);
hipError_t launch_forest_scan_rows(uint64_t* values, size_t rows, size_t n, unsigned long long* totals, uint64_t* tsum, hipStream_t st);

// Trees of one or two BUILT forests gathered into a new compact forest (p252_merkle{4,2}_forest_ragged_select_device_into): nothing is
// hashed, leaves, level blocks and roots move.  The relocation is balanced over tiles of FOREST_SELECT_MOVE_TILE scalars of the new
// arrays, not over trees.
constexpr unsigned FOREST_SELECT_MOVE_TILE = 512;

// one source forest, as its build was given and filled it (n_trees == 0: absent, nothing of it is read)
struct ForestSelectSource {
    const void* leaves = nullptr;
    const void* offsets = nullptr;
    const void* levels = nullptr;
    const void* roots = nullptr;
    size_t n_leaves = 0, n_trees = 0, max_leaves = 0;
};

struct ForestSelectPlan {
    unsigned arity = 4, depth = 0;  // depth of a tree of max_leaves leaves
    size_t n_pick = 0, leaves_cap = 0, max_leaves = 0;  // max_leaves: the larger of the two sources'
    size_t nodes = 0;  // the bound on the new levels: leaves_cap / (arity - 1) + n_pick * depth
    size_t tiles = 0, leaf_tiles = 0, node_tiles = 0;
    size_t index_a_bytes = 0, index_b_bytes = 0, index_new_bytes = 0, work_bytes = 0;
    size_t meta_bytes() const { return index_a_bytes + index_b_bytes + index_new_bytes + work_bytes; }
};
ForestSelectPlan forest_select_plan(unsigned arity, size_t n_trees_a, size_t n_trees_b, size_t max_leaves, size_t n_pick, size_t leaves_cap);

// The whole select on `st`: the indices of A, B and the new forest, the two scans over the picks (the cap rule, d_offsets_new), the
// relocation, the roots.  pick = n_pick uint64 ids (below A.n_trees: of A; then of B); meta = plan.meta_bytes() of scratch, ids and
// counts only.  n_bad (device uint32, may be null) is incremented once per refused pick, whose root is written as zero.
hipError_t launch_forest_select(const ForestSelectPlan& plan, const ForestSelectSource& A, const ForestSelectSource& B, const void* pick,
                                void* leaves_new, void* offsets_new, void* levels_new, void* roots_new, void* n_bad, void* meta,
                                hipStream_t st);

}  // namespace p252
