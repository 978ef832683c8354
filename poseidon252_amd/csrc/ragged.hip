// ragged.hip — n independent sponge hashes of DIFFERENT lengths in one call (p252_hash_ragged*): Hash::digest per message
// (hash.rs:191-195) with io-pattern [Absorb(L_i), Squeeze(out_len)].  Message i = in[offsets[i] .. offsets[i+1]) scalars; its tag
// is tags[L_i - 1], an input like every tag of the library.
//
// Schedule.  A wave runs to its longest lane, so lanes of one wave should absorb the same number of blocks b = ceil(L / 4), and
// the long messages should start first (blocks are dispatched in grid order: the short ones then fill the tail).  Three small
// kernels sort the message indices by b, longest first — a counting sort, no library:
//   k_ragged_hist     per tile of 2,048 messages: bins in LDS, one global atomic per non-empty bin
//   k_ragged_scan     one block: bucket starts, descending bucket order
//   k_ragged_scatter  per tile: LDS rank within the bin, one global atomic per non-empty bin reserves the tile's range
// Buckets: one per b below RAGGED_EXACT_BLOCKS = 1024 (messages of up to 4,092 scalars: every shape of the reference's tests and
// of notes / transactions — no imbalance at all), then 16 per octave of b (a wave's lanes then differ by at most 1/16 of their
// permutations, and such a message runs >= 1,024 permutations, long enough to hide the spread).  The exact range costs one LDS
// counter per b, 1,872 buckets in all = 22 KiB of LDS per sort block.  Bucket 0 takes the bad messages (L == 0, L > max_len,
// decreasing offsets: the unsigned difference wraps above max_len); they sort last and only write zeros.
// The order within a bucket depends on atomic timing; the outputs do not (each lane writes its message's own row).
//
// Sponge.  k_sponge_ragged: one lane per message, the loop of k_sponge (kernels.hip) with a per-lane length and tag.
// k_sponge_ragged_coop: eight lanes per message (coop29.hpp), for launches that cannot fill the chip, under the rule every entry
// point of kernels.hip applies (coop8, kernels.h).  No whole-line fetch variant: the kernel is compute-bound.
//
// The exact-length sort of the encryption calls (k_crypt_ragged_*, crypt_ragged.h) stands here too, behind the sponge: the same two
// passes over one bucket per length.  It hashes nothing; its sponge is k_crypt / k_crypt_coop of kernels.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "blockops.hpp"
#include "coop29.hpp"
#include "crypt_ragged.h"
#include "hades29.hpp"
#include "kernels.h"
#include "ragged.h"

namespace p252 {

namespace {

constexpr unsigned SORT_BLOCK = 256;
constexpr unsigned SORT_ITEMS = 8;  // messages per thread of a sort block
constexpr unsigned SORT_TILE = SORT_BLOCK * SORT_ITEMS;  // (the tile of bucket_hist / bucket_scatter, blockops.hpp)

// absorb blocks of a message of L scalars (no overflow for any L)
__device__ __forceinline__ uint64_t blocks_of(uint64_t L) { return (L >> 2) + ((L & 3u) != 0); }

__device__ __forceinline__ bool bad_len(uint64_t L, uint64_t max_len) { return L == 0 || L > max_len; }

__device__ __forceinline__ unsigned bucket_of(const uint64_t* __restrict__ offsets, size_t i, uint64_t max_len) {
    const uint64_t L = offsets[i + 1] - offsets[i];
    if (bad_len(L, max_len)) return 0;
    const uint64_t b = blocks_of(L);
    if (b < RAGGED_EXACT_BLOCKS) return (unsigned)b;
    const unsigned k = 63u - (unsigned)__clzll((long long)b);  // octave: 10 .. 62
    return RAGGED_EXACT_BLOCKS + (k - 10u) * RAGGED_SUB + (unsigned)((b >> (k - RAGGED_SUB_LOG2)) & (RAGGED_SUB - 1));
}

}  // namespace

// ---- the sort ----
__global__ void __launch_bounds__(SORT_BLOCK) k_ragged_hist(const uint64_t* __restrict__ offsets, size_t n, uint64_t max_len,
                                                            unsigned long long* __restrict__ hist) {
    bucket_hist<SORT_BLOCK, SORT_ITEMS, RAGGED_BUCKETS>(n, hist, [=](size_t i) { return bucket_of(offsets, i, max_len); });
}

// counts -> start of each bucket in the sorted order, buckets in DESCENDING order (longest messages first), in place
__global__ void __launch_bounds__(SORT_BLOCK) k_ragged_scan(unsigned long long* __restrict__ hist) {
    constexpr unsigned PER = (RAGGED_BUCKETS + SORT_BLOCK - 1) / SORT_BLOCK;
    __shared__ unsigned long long part[SORT_BLOCK];
    const unsigned t = threadIdx.x;
    unsigned long long c[PER], sum = 0;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        const unsigned r = t * PER + k;  // rank in descending bucket order
        c[k] = r < RAGGED_BUCKETS ? hist[RAGGED_BUCKETS - 1 - r] : 0ull;
        sum += c[k];
    }
    part[t] = sum;
    __syncthreads();
    for (unsigned off = 1; off < SORT_BLOCK; off <<= 1) {  // inclusive scan of the per-thread sums
        const unsigned long long v = t >= off ? part[t - off] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = t ? part[t - 1] : 0ull;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        const unsigned r = t * PER + k;
        if (r < RAGGED_BUCKETS) hist[RAGGED_BUCKETS - 1 - r] = run;
        run += c[k];
    }
}

__global__ void __launch_bounds__(SORT_BLOCK) k_ragged_scatter(const uint64_t* __restrict__ offsets, size_t n, uint64_t max_len,
                                                               unsigned long long* __restrict__ cursor, uint64_t* __restrict__ order) {
    bucket_scatter<SORT_BLOCK, SORT_ITEMS, RAGGED_BUCKETS>(n, cursor, order, [=](size_t i) { return bucket_of(offsets, i, max_len); });
}

// ---- the sponge, one lane per message: lane i hashes message order[i] (order == null: message i) ----
template <bool TRUNC>
__device__ __forceinline__ void sponge_ragged_body(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags, uint64_t max_len,
                                                   const Scalar32* __restrict__ in, const uint64_t* __restrict__ offsets,
                                                   const uint64_t* __restrict__ order, unsigned out_len, Scalar32* __restrict__ out,
                                                   size_t n, unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t m = order ? order[i] : (uint64_t)i;
    const uint64_t lo = offsets[m];
    const uint64_t len = offsets[m + 1] - lo;
    Scalar32* my_out = out + m * out_len;
    if (bad_len(len, max_len)) {
#pragma unroll 1
        for (unsigned o = 0; o < out_len; ++o) store_zero(my_out + o);
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    const Scalar32* my_in = in + lo;
    E29 s[WIDTH];
    s[0] = load_scalar(tags + (len - 1));
#pragma unroll
    for (int k = 0; k < 4; ++k) s[1 + k] = e29_zero();
    const uint64_t absorb_blocks = blocks_of(len);
    const uint64_t total = absorb_blocks + (out_len + 3) / 4;
#pragma unroll 1
    for (uint64_t it = 0; it < total; ++it) {
        if (it > 0) hades_permute<0x1fu>(s, tab);
        if (it < absorb_blocks) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t e = it * 4 + k;
                if (e < len) add_e(s[1 + k], load_scalar(my_in + e));  // Safe::add, scalar.rs:33-35
            }
        } else {
            const uint64_t ob = (it - absorb_blocks) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ob + k < out_len) store_output<TRUNC>(my_out + ob + k, s[1 + k]);
        }
    }
}

__global__ void __launch_bounds__(P252_BLOCK) k_sponge_ragged(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags, uint64_t max_len,
                                                              const Scalar32* __restrict__ in, const uint64_t* __restrict__ offsets,
                                                              const uint64_t* __restrict__ order, unsigned out_len, Scalar32* __restrict__ out,
                                                              size_t n, unsigned* __restrict__ n_bad) {
    sponge_ragged_body<false>(tab, tags, max_len, in, offsets, order, out_len, out, n, n_bad);
}
__global__ void __launch_bounds__(P252_BLOCK) k_sponge_ragged_trunc(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags,
                                                                    uint64_t max_len, const Scalar32* __restrict__ in,
                                                                    const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ order,
                                                                    unsigned out_len, Scalar32* __restrict__ out, size_t n,
                                                                    unsigned* __restrict__ n_bad) {
    sponge_ragged_body<true>(tab, tags, max_len, in, offsets, order, out_len, out, n, n_bad);
}

// ---- the sponge on a group of eight lanes per message (kernels.hip sponge_coop_body): lane 0 the capacity element, lanes
// 1..4 the rate.  The eight lanes of a group share one message, hence one trip count: a group is active or idle as a whole. ----
template <bool TRUNC>
__device__ __forceinline__ void sponge_ragged_coop_body(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags, uint64_t max_len,
                                                        const Scalar32* __restrict__ in, const uint64_t* __restrict__ offsets,
                                                        const uint64_t* __restrict__ order, unsigned out_len, Scalar32* __restrict__ out,
                                                        size_t n, unsigned* __restrict__ n_bad) {
    const size_t lane = (size_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    const size_t idx = lane / 8;
    if (idx >= n) return;
    const int j = (int)(threadIdx.x & 7u);
    const uint64_t m = order ? order[idx] : (uint64_t)idx;
    const uint64_t lo = offsets[m];
    const uint64_t len = offsets[m + 1] - lo;
    Scalar32* my_out = out + m * out_len;
    if (bad_len(len, max_len)) {
#pragma unroll 1
        for (unsigned o = (unsigned)j; o < out_len; o += 8) store_zero(my_out + o);
        if (n_bad && j == 0) atomicAdd(n_bad, 1u);
        return;
    }
    WaveComm8 cm{j, (int)(((threadIdx.x & 63u) & ~7u) * 4u)};
    CoopLane<8> L = coop_lane<8>(tab, cm);
    const Scalar32* my_in = in + lo;
    const unsigned slot = (unsigned)L.row - 1u;  // my position in the rate (lane 0: none; lanes 5..7 shadow lane 4)
    const bool rate = L.row > 0;
    E29 s, unused;
    if (rate)
        s = slot < len ? load_scalar(my_in + slot) : e29_zero();  // block 0 of the message
    else
        s = load_scalar(tags + (len - 1));
    unused = s;
    const uint64_t absorb_blocks = blocks_of(len);
    const uint64_t total = absorb_blocks + (out_len + 3) / 4;
#pragma unroll 1
    for (uint64_t it = 1; it < total; ++it) {
        hades_permute_coop<8>(s, unused, tab, cm, L);
        if (it < absorb_blocks) {
            const uint64_t e = it * 4 + slot;
            if (rate && e < len) add_e(s, load_scalar(my_in + e));  // Safe::add, scalar.rs:33-35
        } else {
            const uint64_t o = (it - absorb_blocks) * 4 + slot;
            if (rate && j < WIDTH && o < out_len) store_output<TRUNC>(my_out + o, s);
        }
    }
}

__global__ void __launch_bounds__(P252_BLOCK) k_sponge_ragged_coop(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags,
                                                                   uint64_t max_len, const Scalar32* __restrict__ in,
                                                                   const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ order,
                                                                   unsigned out_len, Scalar32* __restrict__ out, size_t n,
                                                                   unsigned* __restrict__ n_bad) {
    sponge_ragged_coop_body<false>(tab, tags, max_len, in, offsets, order, out_len, out, n, n_bad);
}
__global__ void __launch_bounds__(P252_BLOCK) k_sponge_ragged_coop_trunc(const int32_t* __restrict__ tab, const Scalar32* __restrict__ tags,
                                                                         uint64_t max_len, const Scalar32* __restrict__ in,
                                                                         const uint64_t* __restrict__ offsets,
                                                                         const uint64_t* __restrict__ order, unsigned out_len,
                                                                         Scalar32* __restrict__ out, size_t n, unsigned* __restrict__ n_bad) {
    sponge_ragged_coop_body<true>(tab, tags, max_len, in, offsets, order, out_len, out, n, n_bad);
}

// ---- the exact-length sort of the encryption calls (p252_{encrypt,decrypt}_ragged*, crypt_ragged.h): the same two passes over one
// bucket per LENGTH, with every bucket's size rounded up to a whole group of slots ----
__device__ __forceinline__ unsigned crypt_bucket_of(const uint64_t* __restrict__ offsets, size_t i, uint64_t max_len, uint64_t n_scalars) {
    const uint64_t a = offsets[i], b = offsets[i + 1];
    return crypt_span_bad(a, b, max_len, n_scalars) ? 0u : (unsigned)(b - a);  // (max_len <= P252_CRYPT_RAGGED_MAX_LEN: the host refuses more)
}


// the counters to zero and the all-ones sentinel into every slot of the order array, in one launch.  (A kernel, not two
// hipMemsetAsync: replayed from a captured graph, two adjacent memset nodes of different values did not reliably leave zeros in
// the one buffer and ones in the other — the second replay's scatter then started from cursors that were not counts
// (DESIGN.md §3.10).  A kernel node replays like every other launch of the call.)
__global__ void __launch_bounds__(SORT_BLOCK) k_crypt_ragged_clear(unsigned long long* __restrict__ hist, uint64_t* __restrict__ order,
                                                                   size_t slots) {
    const size_t i = (size_t)blockIdx.x * SORT_BLOCK + threadIdx.x;
    if (i < CRYPT_RAGGED_BUCKETS) hist[i] = 0ull;
    if (i < slots) order[i] = CRYPT_RAGGED_SENTINEL;
}

__global__ void __launch_bounds__(SORT_BLOCK) k_crypt_ragged_hist(const uint64_t* __restrict__ offsets, size_t n, uint64_t max_len,
                                                                  uint64_t n_scalars, unsigned long long* __restrict__ hist) {
    bucket_hist<SORT_BLOCK, SORT_ITEMS, CRYPT_RAGGED_BUCKETS>(n, hist, [=](size_t i) { return crypt_bucket_of(offsets, i, max_len, n_scalars); });
}

// counts -> start of each bucket in the sorted order, buckets in DESCENDING order (longest first, bucket 0 last), in place.  Every
// bucket takes its count rounded up to a multiple of `group` slots, so every start is a multiple of `group`.
// (The padded sizes of n counted messages end within the `slots` the order array has.  Counters that add up to more are not what the
// histogram pass leaves; every bucket then starts at 0, where the scatter pass stays below its own count of messages: in bounds.)
__global__ void __launch_bounds__(SORT_BLOCK) k_crypt_ragged_scan(unsigned long long* __restrict__ hist, unsigned group, size_t slots) {
    constexpr unsigned PER = (CRYPT_RAGGED_BUCKETS + SORT_BLOCK - 1) / SORT_BLOCK;
    const unsigned t = threadIdx.x;
    unsigned long long c[PER], sum = 0;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        const unsigned r = t * PER + k;  // rank in descending bucket order
        const unsigned long long cnt = r < CRYPT_RAGGED_BUCKETS ? hist[CRYPT_RAGGED_BUCKETS - 1 - r] : 0ull;
        c[k] = (cnt + group - 1) / group * group;
        sum += c[k];
    }
    unsigned long long total;
    unsigned long long run = block_exclusive<SORT_BLOCK>(sum, &total);
    const bool sane = total <= slots;
    if (!sane) run = 0;
#pragma unroll
    for (unsigned k = 0; k < PER; ++k) {
        const unsigned r = t * PER + k;
        if (r < CRYPT_RAGGED_BUCKETS) hist[CRYPT_RAGGED_BUCKETS - 1 - r] = run;
        if (sane) run += c[k];
    }
}

__global__ void __launch_bounds__(SORT_BLOCK) k_crypt_ragged_scatter(const uint64_t* __restrict__ offsets, size_t n, uint64_t max_len,
                                                                     uint64_t n_scalars, unsigned long long* __restrict__ cursor,
                                                                     uint64_t* __restrict__ order) {
    bucket_scatter<SORT_BLOCK, SORT_ITEMS, CRYPT_RAGGED_BUCKETS>(n, cursor, order,
                                                                 [=](size_t i) { return crypt_bucket_of(offsets, i, max_len, n_scalars); });
}

hipError_t launch_crypt_ragged_schedule(const void* offsets, size_t n, size_t max_len, uint64_t n_scalars, bool coop, void* order, void* hist,
                                        hipStream_t st) {
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    unsigned long long* h = static_cast<unsigned long long*>(hist);
    const unsigned tiles = (unsigned)((n + SORT_TILE - 1) / SORT_TILE);
    const size_t slots = crypt_ragged_slots(n, max_len, coop);
    const size_t cells = slots > CRYPT_RAGGED_BUCKETS ? slots : CRYPT_RAGGED_BUCKETS;
    hipLaunchKernelGGL(k_crypt_ragged_clear, dim3((unsigned)((cells + SORT_BLOCK - 1) / SORT_BLOCK)), dim3(SORT_BLOCK), 0, st, h,
                       static_cast<uint64_t*>(order), slots);
    hipLaunchKernelGGL(k_crypt_ragged_hist, dim3(tiles), dim3(SORT_BLOCK), 0, st, off, n, (uint64_t)max_len, n_scalars, h);
    hipLaunchKernelGGL(k_crypt_ragged_scan, dim3(1), dim3(SORT_BLOCK), 0, st, h, (unsigned)crypt_ragged_group(coop), slots);
    hipLaunchKernelGGL(k_crypt_ragged_scatter, dim3(tiles), dim3(SORT_BLOCK), 0, st, off, n, (uint64_t)max_len, n_scalars, h,
                       static_cast<uint64_t*>(order));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
bool ragged_sort_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("P252_RAGGED_SORT");
        return !(e && e[0] == '0');
    }();
    return on;
}

hipError_t launch_hash_ragged(const int32_t* tab, const void* tags, size_t max_len, const void* in, const void* offsets,
                              unsigned out_len, void* out, size_t n, void* n_bad, void* order, void* hist, hipStream_t st,
                              bool trunc250) {
    if (n == 0) return hipSuccess;
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    const uint64_t* ord = nullptr;
    if (ragged_sort_enabled()) {
        unsigned long long* h = static_cast<unsigned long long*>(hist);
        const unsigned tiles = (unsigned)((n + SORT_TILE - 1) / SORT_TILE);
        hipError_t e = hipMemsetAsync(hist, 0, ragged_hist_bytes(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_ragged_hist, dim3(tiles), dim3(SORT_BLOCK), 0, st, off, n, (uint64_t)max_len, h);
        hipLaunchKernelGGL(k_ragged_scan, dim3(1), dim3(SORT_BLOCK), 0, st, h);
        hipLaunchKernelGGL(k_ragged_scatter, dim3(tiles), dim3(SORT_BLOCK), 0, st, off, n, (uint64_t)max_len, h,
                           static_cast<uint64_t*>(order));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        ord = static_cast<const uint64_t*>(order);
    }
    const bool coop = coop8(n);
    auto k = coop ? (trunc250 ? k_sponge_ragged_coop_trunc : k_sponge_ragged_coop) : (trunc250 ? k_sponge_ragged_trunc : k_sponge_ragged);
    return launch(k, coop ? n * 8 : n, st, tab, static_cast<const Scalar32*>(tags), (uint64_t)max_len, static_cast<const Scalar32*>(in), off,
                  ord, out_len, static_cast<Scalar32*>(out), n, static_cast<unsigned*>(n_bad));
}

}  // namespace p252
