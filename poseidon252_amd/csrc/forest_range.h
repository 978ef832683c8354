// forest_range.h — launch interface between api_forest.cpp and forest_range.hip: m RUNS of leaves [a, a + len) of trees of a ragged
// forest proved and checked in one call (p252_merkle{4,2}_forest_ragged_range_proofs_device_into: data movement only;
// p252_merkle{4,2}_forest_range_verify_device_into).  The proof of a run is byte for byte the shared proof of multiproof.h for the
// positions a .. a + len - 1 of that tree; here it is a closed form of (n_t, a, len): include/poseidon252_hip.h and DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

constexpr unsigned FOREST_RANGE_MAX_DEPTH = 32;  // max_leaves < 2^32: a node index fits in a record word

// p252_merkle{4,2}_forest_range_stride: 2 (arity - 1) depth(max_leaves) scalars, room for the proof of any run
size_t forest_range_stride(unsigned arity, size_t max_leaves);

// The host's view of one call, all derived from (arity, max_leaves, m, k).  bound[l] = the most nodes that the runs of a call have on
// level l together: k for the leaves, min(k + m, k / arity^l + 2 m) above them — what the launches of level l are sized by; the true
// counts stay on the device.
struct ForestRangePlan {
    unsigned arity = 4, log2a = 2, depth = 0;  // depth of a tree of max_leaves leaves
    size_t m = 0, k = 0, max_leaves = 0;
    size_t tiles = 0;  // scan tiles of the runs (forest_scan_rows_tiles)
    size_t bound[FOREST_RANGE_MAX_DEPTH + 1] = {};
    size_t index_bytes = 0;    // the index of the runs: the ragged forest's own over d_leaf_offsets (launch_forest_ragged_index)
    size_t extract_bytes = 0;  // extraction: index_bytes, 16 bytes a run and 8 per 2,048 runs, plus 1 KiB
    size_t verify_bytes = 0;   // verification: index_bytes, (48 + 8 depth) bytes a run, 8 (depth + 1) per 2,048 runs, 20 bytes per
                               // node of level 1's bound, plus 1 KiB
    size_t values_bytes = 0;   // verification: two lists of node values, 64 bytes per node of level 1's bound
};
ForestRangePlan forest_range_plan(unsigned arity, size_t max_leaves, size_t m, size_t k);

// Extraction on `st`, behind the forest's index (ntree, lo: launch_forest_ragged_index): work = plan.extract_bytes of scratch.
// leaves_out and n_bad (uint32) may be null; levels and proof may be null when plan.depth == 0.
hipError_t launch_forest_range_proofs(const ForestRangePlan& plan, const void* leaves, const void* offsets, const void* levels,
                                      const uint64_t* ntree, const uint64_t* lo, size_t n_trees, const void* tree_ids, const void* first,
                                      const void* leaf_offsets, void* leaves_out, void* proof, void* proof_lens, void* counts_out,
                                      void* n_bad, void* work, hipStream_t st);

// Verification on `st`: work = plan.verify_bytes, values = plan.values_bytes of scratch.  proof may be null when proof_stride == 0;
// roots_out, n_hashed (uint64) and n_bad (uint32) may be null.
hipError_t launch_forest_range_verify(const int32_t* tab, const TagArg& tag, const ForestRangePlan& plan, const void* tree_ids,
                                      const void* counts, const void* first, const void* leaf_offsets, const void* leaves_in,
                                      const void* proof, size_t proof_stride, const void* proof_lens, const void* roots, size_t n_trees,
                                      void* ok, void* roots_out, void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st);

}  // namespace p252
