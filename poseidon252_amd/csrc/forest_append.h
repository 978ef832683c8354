// forest_append.h — launch interface between api_forest.cpp and forest_append.hip: leaves appended to the trees of a built forest of trees
// of DIFFERENT sizes, written as a new compact forest (p252_merkle{4,2}_forest_ragged_append_device_into), and the same after each
// tree was cut to its first k_t leaves (p252_merkle{4,2}_forest_ragged_resize_device_into).  Clean nodes are moved, only the nodes
// above a new leaf or a cut are hashed (by forest_update.hip's digest kernels, on lists this unit makes).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "forest_ragged.h"
#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_APPEND_SCAN_TILE = 2048;  // trees per block of the unit's scans
constexpr unsigned FOREST_APPEND_MOVE_TILE = 512;   // scalars (leaves or nodes) per block of the two relocation kernels

// The host's view of one call, all derived from (n_leaves, n_trees, n_add, n_trees_new, max_leaves_new).  N = n_leaves + n_add bounds
// the leaves of the new forest (the old good trees hold at most n_leaves: the build's sum rule; the accepted appends at most n_add:
// this unit's).  Level l (1 .. depth) of the new forest has at most bound[l] = N / arity^l + n_trees_new nodes (ForestRaggedPlan) and
// at most n_add / arity^l + 2 n_trees_new dirty ones (ceil((k + m) / B) - floor(k / B) <= floor(m / B) + 2 for every kept count
// k <= n, the append's k = n included): in[l] = the smaller.
struct ForestAppendPlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    size_t n_trees_old = 0, n_trees = 0, n_leaves_old = 0, n_add = 0, leaves = 0;  // leaves = N
    size_t max_leaves_old = 0, max_leaves = 0, leaves_cap = 0;
    size_t nodes = 0;  // bound of the used part of the new d_levels, in scalars: N / (arity - 1) + n_trees_new * depth
    size_t in[FOREST_RAGGED_MAX_DEPTH + 1] = {};        // most records of level l's dirty list
    size_t list_off[FOREST_RAGGED_MAX_DEPTH + 1] = {};  // where level l's list starts, in records
    size_t tiles = 0, leaf_tiles = 0, node_tiles = 0;
    size_t index_old_bytes = 0, index_new_bytes = 0, work_bytes = 0, list_bytes = 0;
    size_t meta_bytes() const { return index_old_bytes + index_new_bytes + work_bytes; }  // the two indices and the unit's own words
};
ForestAppendPlan forest_append_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t n_add, size_t n_trees_new,
                                    size_t max_leaves_new, size_t leaves_cap);

// The whole call on `st`: meta = plan.meta_bytes() and lists = plan.list_bytes of scratch.  keep (n_trees_new uint64: tree t keeps its
// first min(keep[t], n_t) leaves) is null for an append: every tree whole, plan.n_trees >= plan.n_trees_old.  With keep the new forest
// may have fewer trees than the old one (the trailing ones are dropped), and a call that appends nothing still hashes: at most one
// node per tree and level.  n_bad (uint32) and n_hashed (uint64) may be null; leaves / offsets / levels may be null when the old
// forest has no tree, add when n_add == 0, the levels when no tree of that forest can have one.
hipError_t launch_forest_append(const int32_t* tab, const TagArg& tag, const ForestAppendPlan& plan, const void* leaves, const void* offsets,
                                const void* levels, const void* keep, const void* add, const void* add_offsets, void* leaves_new,
                                void* offsets_new, void* levels_new, void* roots, void* n_bad, void* n_hashed, void* meta, void* lists,
                                hipStream_t st);

// The unit's scans over the trees for a caller that made the per-tree words itself (forest_frontier.hip: the same trees, the same
// rules, no old forest): nold[t] = n_t, madd[t] = m_t or FOREST_APPEND_REFUSED, both n_trees uint64.  rows = (depth + 1) x
// (n_trees + 1) uint64, tsum = (depth + 1) x tiles, tiles = ceil(n_trees / FOREST_APPEND_SCAN_TILE).
constexpr uint64_t FOREST_APPEND_REFUSED = ~0ull;  // m_t of an append refused before the sum rule
struct ForestAppendScan {
    uint64_t* nold = nullptr;
    uint64_t* madd = nullptr;
    uint64_t* rows = nullptr;
    uint64_t* tsum = nullptr;
    size_t n_trees = 0, tiles = 0;
    uint64_t n_add = 0;
    unsigned log2a = 2, depth = 0;
};
// the sum rule: madd[t] becomes the accepted m_t (0 for a refused append).  never_zero = n_trees words, none of them 0, in the place
// of the kept counts: no tree is empty to this scan, so it writes no root and counts nothing.
hipError_t forest_append_scan_sum_rule(const ForestAppendScan& scan, const uint64_t* never_zero, hipStream_t st);
// every level's dirty list of trees that keep all of their n_t leaves: rows[l][t] = where tree t's records start in list l (rows[l]
// [n_trees] = the list's count), and record g of list l = (tree, floor(n_t / a^l) + g - rows[l][t]) in the 16-byte format of
// forest_update.hip at lists[list_off[l] + g], for g < in[l] (l = 1 .. depth)
hipError_t forest_append_scan_dirty_lists(const ForestAppendScan& scan, const size_t* in, const size_t* list_off, void* lists, hipStream_t st);

}  // namespace p252
