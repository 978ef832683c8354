// blockops.hpp — the bookkeeping primitives of the ragged calls (ragged.hip, forest_ragged.hip, forest_openings.hip, forest_update.hip,
// forest_journal.hip, forest_append.hip, multiproof.hip, forest_multiproof.hip), one definition each: the block scan and the row scan
// of tile sums, the search of a tree in ascending starts, the claim table with its wave append, and the two passes of a counting
// sort.  Device code only, and nothing of the permutation: the hashing side of the same files is forest_node.hpp.  Every __global__
// kernel stays in its own file under its own name (no relocatable device code in this build); only the bodies come from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace p252 {

// ---- scans ----
// exclusive scan of one value per thread over a block of BLOCK threads (returns the block total in *total)
template <unsigned BLOCK, class T>
__device__ __forceinline__ T block_exclusive(T v, T* total) {
    __shared__ T part[BLOCK];
    const unsigned t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (unsigned off = 1; off < BLOCK; off <<= 1) {
        const T o = t >= off ? part[t - off] : (T)0;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    const T incl = part[t];
    *total = part[BLOCK - 1];
    __syncthreads();  // (part is reused by the caller's next call)
    return incl - v;
}

// one block: the tile sums of a row -> their exclusive scan, in place.  BLOCK tiles a trip of the loop, `carry` from trip to trip: the
// second trip starts past BLOCK tiles (of 2,048 trees in all three callers: past 524,288 trees)
template <unsigned BLOCK, class T>
__device__ __forceinline__ void scan_tile_row(T* __restrict__ row, size_t tiles) {
    T carry = 0;
#pragma unroll 1
    for (size_t base = 0; base < tiles; base += BLOCK) {
        const size_t i = base + threadIdx.x;
        const T v = i < tiles ? row[i] : (T)0;
        T total;
        const T ex = block_exclusive<BLOCK>(v, &total);
        if (i < tiles) row[i] = carry + ex;
        carry += total;
    }
}

// ---- the search ----
// the largest t in [lo, hi] with B[t] <= g (B ascending, B[lo] <= g): of trees that start at the same place, the last — the one that
// holds g when g is below the total
__device__ __forceinline__ size_t last_at_or_below(const uint64_t* __restrict__ B, size_t lo, size_t hi, uint64_t g) {
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) >> 1;
        if (B[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- the claim table: open addressing, linear probing, a power of two of slots (>= CLAIM_MIN_SLOTS, >= twice the keys offered, so
// at most half full), cleared to 0xFF bytes; a key is a slot number of the forest, and no slot has the number CLAIM_EMPTY ----
constexpr unsigned long long CLAIM_EMPTY = ~0ull;
constexpr size_t CLAIM_MIN_SLOTS = 64;

// empty -> key in a table of 2^(64 - shift) slots, with one 64-bit compare-and-swap per probe: true for the one lane that installs
// the key
__device__ __forceinline__ bool claim(unsigned long long* __restrict__ table, unsigned shift, unsigned long long key) {
    const size_t mask = ((size_t)1 << (64 - shift)) - 1;
    size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> shift);
    for (;;) {  // (the table is at most half full: an empty slot is met)
        const unsigned long long seen = atomicCAS(table + h, CLAIM_EMPTY, key);
        if (seen == CLAIM_EMPTY) return true;
        if (seen == key) return false;
        h = (h + 1) & mask;
    }
}

// the wave's winners (winners = __ballot(won), not zero) take consecutive places behind *count, with one atomic add per wave: ballot,
// popcount, the leader's base broadcast.  Returns the place of this lane (valid where won).  The whole wave calls this: no early
// return before it.
__device__ __forceinline__ unsigned long long append_place(bool won, unsigned long long winners, unsigned long long* __restrict__ count) {
    const unsigned lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)winners) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(winners));
    base = __shfl(base, leader);
    return base + __popcll(winners & ((1ull << lane) - 1));
}

// ---- a counting sort of n items into BINS buckets, tiles of BLOCK * ITEMS items per block; bucket_fn(i) < BINS is item i's bucket.
// Between the two passes the caller turns the counts into the buckets' starts, in the order it wants.  The order within a bucket
// depends on atomic timing. ----
// bins in LDS, one global atomic per non-empty bin
template <unsigned BLOCK, unsigned ITEMS, unsigned BINS, class F>
__device__ __forceinline__ void bucket_hist(size_t n, unsigned long long* __restrict__ hist, F bucket_fn) {
    __shared__ unsigned cnt[BINS];
    for (unsigned b = threadIdx.x; b < BINS; b += BLOCK) cnt[b] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * (BLOCK * ITEMS) + threadIdx.x;
#pragma unroll
    for (unsigned k = 0; k < ITEMS; ++k) {
        const size_t i = t0 + (size_t)k * BLOCK;
        if (i < n) atomicAdd(&cnt[bucket_fn(i)], 1u);
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < BINS; b += BLOCK)
        if (cnt[b]) atomicAdd(&hist[b], (unsigned long long)cnt[b]);
}

// the LDS rank within the bin, one global atomic per non-empty bin reserves the tile's range behind cursor[bin]; order[place] = item
// (the bins partition 0 .. n-1: every slot below n, written once)
template <unsigned BLOCK, unsigned ITEMS, unsigned BINS, class F>
__device__ __forceinline__ void bucket_scatter(size_t n, unsigned long long* __restrict__ cursor, uint64_t* __restrict__ order, F bucket_fn) {
    __shared__ unsigned cnt[BINS];
    __shared__ unsigned long long base[BINS];
    for (unsigned b = threadIdx.x; b < BINS; b += BLOCK) cnt[b] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * (BLOCK * ITEMS) + threadIdx.x;
    unsigned bk[ITEMS], rk[ITEMS];
#pragma unroll
    for (unsigned k = 0; k < ITEMS; ++k) {
        const size_t i = t0 + (size_t)k * BLOCK;
        bk[k] = i < n ? bucket_fn(i) : 0u;
        rk[k] = i < n ? atomicAdd(&cnt[bk[k]], 1u) : 0u;
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < BINS; b += BLOCK)
        if (cnt[b]) base[b] = atomicAdd(&cursor[b], (unsigned long long)cnt[b]);
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < ITEMS; ++k) {
        const size_t i = t0 + (size_t)k * BLOCK;
        if (i < n) order[base[bk[k]] + rk[k]] = i;
    }
}

}  // namespace p252
