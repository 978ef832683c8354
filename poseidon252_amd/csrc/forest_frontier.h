// forest_frontier.h — launch interface between api_forest.cpp and forest_frontier.hip: leaves appended to a forest of Merkle trees that is
// kept ONLY as its frontiers (p252_merkle{4,2}_forest_frontier_append_device: per tree a leaf count, a root and (depth + 1) rows of
// arity - 1 scalars, updated in place), and that state taken out of a built ragged forest
// (p252_merkle{4,2}_forest_frontier_extract_device_into: data movement only).  The digests of an append run on multiproof.hip's
// kernels, over records this unit makes; the frontier is their `proof`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "forest_append.h"
#include "forest_ragged.h"
#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_FRONTIER_BLOCK = 256;      // threads of a bookkeeping block

// The host's view of one append, all derived from (arity, n_trees, max_leaves, n_add).  depth = D(max_leaves); a tree's frontier is
// rows 0 .. depth of arity - 1 scalars: stride = (depth + 1) (arity - 1).  Level l (1 .. depth) computes at most in[l] = n_add /
// arity^l + 2 min(n_trees, n_add) nodes over all trees (ceil((n + m) / B) - floor(n / B) <= floor(m / B) + 2 per tree that grows, and
// the accepted appends never add up to more than n_add: the sum rule); list_off[l] = where level l's records, widths and values start.
struct ForestFrontierPlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    size_t n_trees = 0, n_add = 0, max_leaves = 0, stride = 0;
    size_t in[FOREST_RAGGED_MAX_DEPTH + 1] = {};
    size_t list_off[FOREST_RAGGED_MAX_DEPTH + 1] = {};
    size_t records = 0, tiles = 0;
    size_t tree_bytes = 0;  // three words per tree, one scan row per level (row 0 unused), the scans' tile sums (forest_append.hip's scans)
    size_t work_bytes() const { return tree_bytes + records * 16 + ((records * 4 + 255) & ~(size_t)255); }  // + records and widths
    size_t value_bytes() const { return records * 32; }                                                    // the V_l of every level
};
size_t forest_frontier_stride(unsigned arity, size_t max_leaves);  // p252_merkle{4,2}_forest_frontier_bound
ForestFrontierPlan forest_frontier_plan(unsigned arity, size_t n_trees, size_t max_leaves, size_t n_add);

// What an append holds between its last digest launch and k_ff_finish, for a pass that reads it there (forest_witness.hip): per tree
// n_t and the accepted m_t; rows[l][t] = where tree t's run of V_l = the nodes [f_l(n), c_l(n')) starts inside level l's values, which
// begin at values + list_off[l] (l >= 1; V_0 = add + add_offsets[t]); the frontier with its OLD rows.  rows, values and add are read for
// a tree with m_t > 0 only.
struct ForestFrontierView {
    const uint64_t* nold = nullptr;
    const uint64_t* madd = nullptr;
    const uint64_t* rows = nullptr;  // (depth + 1) x (n_trees + 1)
    uint64_t list_off[FOREST_RAGGED_MAX_DEPTH + 1] = {};
    const void* values = nullptr;
    const void* add = nullptr;
    const uint64_t* add_offsets = nullptr;
    const void* frontier = nullptr;
    uint64_t stride = 0;  // scalars of one tree's frontier
    size_t n_trees = 0;
    unsigned log2a = 2, depth = 0;
};
struct ForestWitnesses;  // forest_witness.h

// The whole append on `st`: work = plan.work_bytes(), values = plan.value_bytes() of scratch.  counts (n_trees uint64), frontier
// (n_trees x plan.stride scalars) and roots (n_trees scalars) are read and, once every digest launch is queued, updated in place.
// add may be null when plan.n_add == 0; n_bad (uint32) and n_hashed (uint64) may be null.  witnesses (null: none, and no launch for
// them) are refreshed behind the last digest launch and before the state changes (launch_forest_witness_refresh).
hipError_t launch_forest_frontier_append(const int32_t* tab, const TagArg& tag, const ForestFrontierPlan& plan, void* counts, void* frontier,
                                         void* roots, const void* add, const void* add_offsets, void* n_bad, void* n_hashed, void* work,
                                         void* values, const ForestWitnesses* witnesses, hipStream_t st);

// The state of a built ragged forest on `st`: meta = forest_ragged_index_bytes(n_trees) of scratch; the leaf counts are the build's
// own validation (launch_forest_ragged_index).  A bad tree gets count 0, zero rows and a zero root and is counted in n_bad (uint32,
// may be null).  levels may be null when max_leaves_forest <= 1.  Nothing is hashed.
hipError_t launch_forest_frontier_extract(unsigned arity, const void* leaves, size_t n_leaves, const void* offsets, size_t n_trees,
                                          size_t max_leaves_forest, const void* levels, const void* roots_forest, size_t max_leaves,
                                          void* counts, void* frontier, void* roots, void* n_bad, void* meta, hipStream_t st);

}  // namespace p252
