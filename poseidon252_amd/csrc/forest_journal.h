// forest_journal.h — launch interface between api_forest.cpp and forest_journal.hip: the journaled leaf update of a ragged forest
// (p252_merkle{4,2}_forest_ragged_update_journaled_device_into: the update of forest_update.h that first saves every leaf and node it
// overwrites) and the swap that undoes, and then redoes, it without one digest (p252_merkle{4,2}_forest_ragged_journal_swap_device_into).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "forest_update.h"

namespace p252 {

// The update's plan (forest_update.h) and a claim table for level 0: the (tree, leaf) pairs go through it as every upper level's
// nodes do, so a power of two >= max(64, 2 k) slots — also when the forest has no level above its leaves.  bound = the most
// journal entries one call writes: the sum of up.in[0 .. depth], SIZE_MAX when that overflows.
struct ForestJournalPlan {
    ForestUpdatePlan up;
    size_t slots0 = 0;
    size_t table_bytes = 0;  // the widest table, level 0's included
    size_t bound = 0;
};
ForestJournalPlan forest_journal_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);
// bound alone, for any sizes (no plan is made: 0 for a zero size, SIZE_MAX on overflow)
size_t forest_journal_bound(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);

// The caller's journal: entry g < *len = (ids[g], values[2 g], values[2 g + 1]); cap = its capacity in entries.
struct ForestJournal {
    void* ids = nullptr;     // uint4 {tree id, level + 1, node index low, node index high}; all zero: void
    void* values = nullptr;  // 32 bytes per entry
    size_t cap = 0;
    void* len = nullptr;     // device uint64
};

// The whole journaled update on `st`, arguments as launch_forest_update; table = plan.table_bytes of scratch.  j.cap >= plan.bound
// is the caller's check.  *j.len is set, not added to.
hipError_t launch_forest_update_journaled(const int32_t* tab, const TagArg& tag, const ForestJournalPlan& plan, void* leaves,
                                          const void* offsets, const uint64_t* ntree, const uint64_t* lo, void* levels, const void* tree_ids,
                                          const void* leaf_ids, const void* new_leaves, void* roots, void* n_bad, void* n_hashed,
                                          const ForestJournal& j, void* ids, void* table, hipStream_t st);

// Entry g < min(*j.len, j.cap) exchanges its 32 bytes with the node it names; an entry that names no node of this forest writes
// nothing and is counted in *n_bad (uint32, may be null, as roots).  ntree / lo: the forest's index.
hipError_t launch_forest_journal_swap(unsigned arity, void* leaves, const void* offsets, const uint64_t* ntree, const uint64_t* lo,
                                      size_t n_trees, void* levels, const ForestJournal& j, void* roots, void* n_bad, hipStream_t st);

}  // namespace p252
