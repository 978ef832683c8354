// ragged.h — launch interface between api.cpp and ragged.hip: n sponge hashes of DIFFERENT lengths in one call
// (p252_hash_ragged*).  Message i = in[offsets[i] .. offsets[i+1]) scalars; tags[L - 1] is the tag of a message of length L.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace p252 {

// the schedule's key: absorb blocks b = ceil(L / 4), one bucket per b below RAGGED_EXACT_BLOCKS, then RAGGED_SUB buckets per
// octave of b; bucket 0 holds the bad messages (L == 0, L > max_len, decreasing offsets), which sort last
constexpr unsigned RAGGED_EXACT_BLOCKS = 1024;
constexpr unsigned RAGGED_SUB_LOG2 = 4;
constexpr unsigned RAGGED_SUB = 1u << RAGGED_SUB_LOG2;
constexpr unsigned RAGGED_BUCKETS = RAGGED_EXACT_BLOCKS + (62 - 10 + 1) * RAGGED_SUB;  // octaves 2^10 .. 2^62 of b: 1,872

// P252_RAGGED_SORT=0 (read once per process): the sponge runs over the identity order and needs no scratch
bool ragged_sort_enabled();
// scratch of the sort: order = n uint64 message indices, hist = RAGGED_BUCKETS uint64 counters (both unused when the sort is off)
inline size_t ragged_order_bytes(size_t n) { return n * sizeof(uint64_t); }
inline size_t ragged_hist_bytes() { return (size_t)RAGGED_BUCKETS * sizeof(uint64_t); }

// sort (when enabled) + sponge on `st`.  n_bad (device uint32, may be null) is incremented once per bad message, whose
// out_len output scalars are written as zero.  trunc250: finalize_truncated's raw limbs instead of BlsScalars.
hipError_t launch_hash_ragged(const int32_t* tab, const void* tags, size_t max_len, const void* in, const void* offsets,
                              unsigned out_len, void* out, size_t n, void* n_bad, void* order, void* hist, hipStream_t st,
                              bool trunc250);

}  // namespace p252
