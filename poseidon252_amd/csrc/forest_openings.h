// forest_openings.h — launch interface between api_forest.cpp and forest_openings.hip: openings out of a forest of trees of DIFFERENT
// sizes (p252_merkle{4,2}_forest_ragged_openings_device), their re-hash with a depth per opening
// (p252_merkle{4,2}_path_ragged_device) and the comparison with a root per opening (p252_merkle{4,2}_forest_ragged_verify_device).
// Layout of k openings at stride D: leaves[k], siblings[k][D][arity - 1], positions[k][D], depths[k] (uint8; rows l >= depths[i]
// are zero; FOREST_OPENINGS_BAD_DEPTH marks a bad opening).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_OPENINGS_MAX_DEPTH = 64;
constexpr unsigned FOREST_OPENINGS_BAD_DEPTH = 0xFF;
constexpr unsigned FOREST_OPENINGS_BINS = FOREST_OPENINGS_MAX_DEPTH + 2;  // depths 0 .. 64, then the bad ones

// scratch: one 32-byte record per opening (extraction); the sort's order (k uint64) and bin counters (both unused with
// P252_RAGGED_SORT=0)
inline size_t forest_openings_record_bytes(size_t k) { return k * 32; }
inline size_t forest_openings_order_bytes(size_t k) { return k * sizeof(uint64_t); }
inline size_t forest_openings_hist_bytes() { return (size_t)FOREST_OPENINGS_BINS * sizeof(uint64_t); }

// extraction, no hashing: ntree / lo = the forest's index (launch_forest_ragged_index), records = forest_openings_record_bytes(k)
// of scratch.  A bad opening (tree id >= n_trees, a bad tree, leaf id >= n_t) is written as zeros with depth 0xFF and counted
// once in *n_bad (device uint32, may be null).  leaves must hold at least one scalar.
hipError_t launch_forest_openings(unsigned arity, const void* leaves, const void* levels, const void* offsets, const uint64_t* ntree,
                                  const uint64_t* lo, size_t n_trees, const void* tree_ids, const void* leaf_ids, size_t k,
                                  unsigned stride_depth, void* records, void* leaves_out, void* siblings, void* positions, void* depths,
                                  void* n_bad, hipStream_t st);

// the second half of that extraction alone, for a caller that writes the records itself (forest_consistency.hip): records[i] =
// {leaf start of the tree, n_t (0: nothing to open, all of opening i is written as zero), LO[t], leaf id} as k_fo_record lays them out
hipError_t launch_forest_opening_pieces(unsigned arity, const void* leaves, const void* levels, const void* records, size_t k,
                                        unsigned stride_depth, void* leaves_out, void* siblings, void* positions, hipStream_t st);

// the depth sort alone: order[0 .. k) = the openings deepest first, those with depths[i] > stride_depth last; order =
// forest_openings_order_bytes(k) and hist = forest_openings_hist_bytes() of scratch
hipError_t launch_forest_depth_sort(const void* depths, size_t k, unsigned stride_depth, void* order, void* hist, hipStream_t st);

// roots[i] = the re-hash of the first depths[i] levels of opening i; depths[i] > stride_depth: a zero root, counted in *n_bad.
// order / hist: the depth sort's scratch, or null for the identity order.
hipError_t launch_path_ragged(unsigned arity, const int32_t* tab, const TagArg& tag, const void* leaves, const void* siblings,
                              const void* positions, const void* depths, unsigned stride_depth, void* roots, size_t k, void* n_bad,
                              void* order, void* hist, hipStream_t st);

// ok[i] = 1 iff depths[i] <= stride_depth, tree_ids[i] < n_trees and roots[i] == expected[tree_ids[i]]
hipError_t launch_compare_roots_gather(const void* roots, const void* depths, unsigned stride_depth, const void* tree_ids,
                                       const void* expected, size_t n_trees, void* ok, size_t k, hipStream_t st);

}  // namespace p252
