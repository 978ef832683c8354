// pairs.hip — the stable sort and the de-duplication of k (tree id, leaf id) pairs on the device: d_order of the sequential updates,
// the ascending distinct pairs of the shared proofs.  The key of pair i is the 96-bit number (tree id, leaf id), both parts unsigned,
// nothing assumed about the values; ties keep their index order.
//
// The method is a least-significant-digit radix sort over the 12 bytes of the key (PAIRS_PASSES; bytes 0 .. 7 of the leaf id, then
// bytes 0 .. 3 of the tree id), on 16-byte records {tree, index, leaf low, leaf high} that ping-pong between two arrays, one dwordx4
// per lane.  A TILE is PAIRS_TILE neighbours of the list, one block; a block takes its tile in PAIRS_ROUNDS rounds of PAIRS_BLOCK
// neighbours, lane by lane in the list's order.
//   k_po_load        one lane per pair: the record into array 0, and the OR of key ^ key[0] over all pairs into three control words
//   k_po_plan        one lane: a digit whose byte of that OR is zero has the same value in every key, and its pass would move
//                    nothing: the pass is SKIPPED — its three kernels leave at once on the plan's word.  The plan holds per pass
//                    whether it runs, which array it reads (the ping-pong parity, a device word: the host never learns which passes
//                    ran) and whether it is the last to run.  Keys that are all equal keep pass 0, which then is the identity.
//   per pass:
//   k_po_count       one block per tile: the tile's count of every digit value, digit-major (counts[digit][tile])
//   k_po_scan        one block per digit value: the exclusive scan of that value's row over the tiles, in trips of PAIRS_SCAN_BLOCK
//                    tiles with a carry, and the row's total
//   k_po_scatter     one block per tile: the place of a record = the start of its digit value (an exclusive scan of the 256 totals,
//                    done by every block for itself) + the value's count in the tiles before + its RANK among the tile's records of
//                    that value.  The rank is what makes the pass stable, and it is computed, never claimed: inside a wave the lanes
//                    of one value are found by eight ballots (one per bit of the digit) and the rank is the popcount of the matching
//                    lanes below; across the four waves of a round the per-wave counts lie in LDS and are added in wave order;
//                    across rounds a per-value running count.  (An LDS atomicAdd would hand the ranks out in arrival order.)
//                    The last pass that runs writes the indices straight into d_order; for the de-duplication it writes records.
//   the de-duplication, on the sorted records:
//   k_po_heads       one block per tile: the number of HEADS — records whose key differs from their predecessor's
//   k_po_scan_heads  one block: the exclusive scan of those numbers, in trips with a carry, and *d_n_unique
//   k_po_compact     one block per tile: head number h of the list goes to entry h of every output; stability put the lowest index
//                    of a pair at its head, and that index is d_first
// A pass is three launches ordered by the stream: no block ever waits for another, there is no look-back and no flag one block sets
// for another to poll.  The number and the grids of the launches depend on k alone.
#include <hip/hip_runtime.h>

#include "pairs.h"

namespace p252 {

namespace {

constexpr unsigned PO_WAVES = PAIRS_BLOCK / 64;
// the control words
constexpr unsigned PO_DIFF = 0;     // [3]: OR of key ^ key[0]: leaf low, leaf high, tree
constexpr unsigned PO_ACTIVE = 4;   // [12]: the pass runs
constexpr unsigned PO_SOURCE = 16;  // [12]: the array the pass reads
constexpr unsigned PO_LAST = 28;    // [12]: the pass is the last that runs
constexpr unsigned PO_FINAL = 40;   // the array that holds the sorted records when the last pass wrote records
constexpr size_t PO_CTL_BYTES = 256;

// digit p of a record {tree, index, leaf low, leaf high}
__device__ __forceinline__ unsigned digit_of(const uint4 r, unsigned p) {
    const unsigned word = p < 4 ? r.z : p < 8 ? r.w : r.x;
    return (word >> ((p & 3u) * 8u)) & 0xffu;
}

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << lane_id()) - 1ull; }

// the sum of v over the lanes of the wave at and below this one
__device__ __forceinline__ unsigned wave_inclusive(unsigned v) {
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(v, d);
        if (lane_id() >= d) v += up;
    }
    return v;
}

// `mine` is the same in all lanes of a wave: the sum of it over the waves before this one, and over all waves into `total`.
// ws: PO_WAVES words of LDS; two barriers, so every lane of the block comes here.
__device__ __forceinline__ unsigned waves_before(unsigned mine, unsigned* ws, unsigned& total) {
    const unsigned wave = threadIdx.x >> 6;
    if (lane_id() == 0) ws[wave] = mine;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < PO_WAVES; ++w) {
        const unsigned c = ws[w];
        before += w < wave ? c : 0u;
        all += c;
    }
    __syncthreads();
    total = all;
    return before;
}

// one trip of a scan over the tiles: the exclusive sum of v over the lanes of the block before this one; the block's sum into total
__device__ __forceinline__ unsigned trip_exclusive(unsigned v, unsigned* ws, unsigned& total) {
    const unsigned incl = wave_inclusive(v);
    const unsigned wave_sum = __shfl(incl, 63);
    return waves_before(wave_sum, ws, total) + incl - v;
}

}  // namespace

// ---- the records, and what varies ----
__global__ void __launch_bounds__(PAIRS_BLOCK) k_po_load(const uint32_t* __restrict__ tree_ids, const uint64_t* __restrict__ leaf_ids, uint32_t k,
                                                         uint4* __restrict__ recs, unsigned* __restrict__ ctl) {
    const size_t i = (size_t)blockIdx.x * PAIRS_BLOCK + threadIdx.x;
    const bool valid = i < k;
    const uint64_t leaf0 = leaf_ids[0];
    const uint32_t tree0 = tree_ids ? tree_ids[0] : 0u;
    unsigned lo = 0, hi = 0, tr = 0;
    if (valid) {
        const uint64_t leaf = leaf_ids[i];
        const uint32_t tree = tree_ids ? tree_ids[i] : 0u;
        recs[i] = make_uint4(tree, (uint32_t)i, (uint32_t)leaf, (uint32_t)(leaf >> 32));
        lo = (uint32_t)(leaf ^ leaf0);
        hi = (uint32_t)((leaf ^ leaf0) >> 32);
        tr = tree ^ tree0;
    }
#pragma unroll
    for (unsigned d = 32; d > 0; d >>= 1) {
        lo |= __shfl_xor(lo, d);
        hi |= __shfl_xor(hi, d);
        tr |= __shfl_xor(tr, d);
    }
    if (lane_id() == 0) {
        if (lo) atomicOr(&ctl[PO_DIFF + 0], lo);
        if (hi) atomicOr(&ctl[PO_DIFF + 1], hi);
        if (tr) atomicOr(&ctl[PO_DIFF + 2], tr);
    }
}

__global__ void k_po_plan(unsigned* __restrict__ ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned lo = ctl[PO_DIFF + 0], hi = ctl[PO_DIFF + 1], tr = ctl[PO_DIFF + 2];
    unsigned varies = 0;
#pragma unroll
    for (unsigned p = 0; p < PAIRS_PASSES; ++p) {
        const unsigned word = p < 4 ? lo : p < 8 ? hi : tr;
        if ((word >> ((p & 3u) * 8u)) & 0xffu) varies |= 1u << p;
    }
    if (!varies) varies = 1u;  // all keys equal: pass 0 runs, and is the identity
    unsigned parity = 0;
#pragma unroll
    for (unsigned p = 0; p < PAIRS_PASSES; ++p) {
        const unsigned on = (varies >> p) & 1u;
        ctl[PO_ACTIVE + p] = on;
        ctl[PO_SOURCE + p] = parity;
        ctl[PO_LAST + p] = on && (varies >> (p + 1)) == 0;
        parity ^= on;
    }
    ctl[PO_FINAL] = parity;
}

// ---- one pass ----
__global__ void __launch_bounds__(PAIRS_BLOCK) k_po_count(const uint4* __restrict__ recs0, const uint4* __restrict__ recs1,
                                                          const unsigned* __restrict__ ctl, unsigned pass, uint32_t k,
                                                          unsigned* __restrict__ counts, unsigned n_tiles) {
    if (!ctl[PO_ACTIVE + pass]) return;
    __shared__ unsigned hist[PAIRS_DIGITS];
    const uint4* __restrict__ src = ctl[PO_SOURCE + pass] ? recs1 : recs0;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t start = (size_t)blockIdx.x * PAIRS_TILE + threadIdx.x;
#pragma unroll 2
    for (unsigned r = 0; r < PAIRS_ROUNDS; ++r) {
        const size_t i = start + (size_t)r * PAIRS_BLOCK;
        if (i < k) atomicAdd(&hist[digit_of(src[i], pass)], 1u);  // (a count, not a rank: the sum does not depend on the arrival order)
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
}

__global__ void __launch_bounds__(PAIRS_SCAN_BLOCK) k_po_scan(const unsigned* __restrict__ ctl, unsigned pass, unsigned* __restrict__ counts,
                                                              unsigned n_tiles, unsigned* __restrict__ totals) {
    if (!ctl[PO_ACTIVE + pass]) return;
    __shared__ unsigned ws[PO_WAVES];
    unsigned* __restrict__ row = counts + (size_t)blockIdx.x * n_tiles;
    unsigned carry = 0;
#pragma unroll 1
    for (unsigned base = 0; base < n_tiles; base += PAIRS_SCAN_BLOCK) {
        const unsigned t = base + threadIdx.x;
        const unsigned v = t < n_tiles ? row[t] : 0u;
        unsigned total;
        const unsigned before = trip_exclusive(v, ws, total);
        if (t < n_tiles) row[t] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(PAIRS_BLOCK) k_po_scatter(uint4* recs0, uint4* recs1, const unsigned* __restrict__ ctl, unsigned pass,
                                                            uint32_t k, const unsigned* __restrict__ counts, unsigned n_tiles,
                                                            const unsigned* __restrict__ totals, uint32_t* __restrict__ order) {
    if (!ctl[PO_ACTIVE + pass]) return;
    // wave_count[w][d]: row w is written by wave w alone; lane d of the block folds column d, one bank per lane
    __shared__ unsigned place[PAIRS_DIGITS];
    __shared__ unsigned wave_count[PO_WAVES][PAIRS_DIGITS];
    __shared__ unsigned ws[PO_WAVES];
    const unsigned source = ctl[PO_SOURCE + pass];
    const uint4* __restrict__ src = source ? recs1 : recs0;
    uint4* __restrict__ dst = source ? recs0 : recs1;
    const bool indices_only = order != nullptr && ctl[PO_LAST + pass];
    const unsigned wave = threadIdx.x >> 6;
    {
        unsigned unused;
        const unsigned digit_start = trip_exclusive(totals[threadIdx.x], ws, unused);
        place[threadIdx.x] = digit_start + counts[(size_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (unsigned w = 0; w < PO_WAVES; ++w) wave_count[w][threadIdx.x] = 0;
    }
    __syncthreads();
    const size_t start = (size_t)blockIdx.x * PAIRS_TILE + threadIdx.x;
#pragma unroll 1
    for (unsigned r = 0; r < PAIRS_ROUNDS; ++r) {
        const size_t i = start + (size_t)r * PAIRS_BLOCK;
        const bool valid = i < k;
        const uint4 rec = valid ? src[i] : make_uint4(0u, 0u, 0u, 0u);
        const unsigned d = digit_of(rec, pass);
        // the lanes of this wave that hold a record of digit value d
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (unsigned b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long with_bit = __ballot(bit);
            same &= bit ? with_bit : ~with_bit;
        }
        const unsigned rank = __popcll(same & lanes_below());
        if (valid && rank == 0) wave_count[wave][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            unsigned before = 0;
#pragma unroll
            for (unsigned w = 0; w + 1 < PO_WAVES; ++w) before += w < wave ? wave_count[w][d] : 0u;
            const unsigned at = place[d] + before + rank;
            if (at < k) {  // (it is, by the counts; a record is never written outside the arrays)
                if (indices_only)
                    order[at] = rec.y;
                else
                    dst[at] = rec;
            }
        }
        __syncthreads();
        {  // lane d of the block: this round's records of digit value d are placed
            unsigned sum = 0;
#pragma unroll
            for (unsigned w = 0; w < PO_WAVES; ++w) {
                sum += wave_count[w][threadIdx.x];
                wave_count[w][threadIdx.x] = 0;
            }
            place[threadIdx.x] += sum;
        }
        __syncthreads();
    }
}

// ---- the de-duplication ----
namespace {
__device__ __forceinline__ bool is_head(const uint4* __restrict__ recs, size_t i, const uint4 rec) {
    if (i == 0) return true;
    const uint4 prev = recs[i - 1];
    return prev.x != rec.x || prev.z != rec.z || prev.w != rec.w;
}
}  // namespace

__global__ void __launch_bounds__(PAIRS_BLOCK) k_po_heads(const uint4* __restrict__ recs0, const uint4* __restrict__ recs1,
                                                          const unsigned* __restrict__ ctl, uint32_t k, unsigned* __restrict__ heads) {
    __shared__ unsigned ws[PO_WAVES];
    const uint4* __restrict__ recs = ctl[PO_FINAL] ? recs1 : recs0;
    const size_t start = (size_t)blockIdx.x * PAIRS_TILE + threadIdx.x;
    unsigned n = 0;
#pragma unroll 1
    for (unsigned r = 0; r < PAIRS_ROUNDS; ++r) {
        const size_t i = start + (size_t)r * PAIRS_BLOCK;
        const bool head = i < k && is_head(recs, i, recs[i]);
        n += __popcll(__ballot(head));
    }
    unsigned total;
    waves_before(n, ws, total);
    if (threadIdx.x == 0) heads[blockIdx.x] = total;
}

__global__ void __launch_bounds__(PAIRS_SCAN_BLOCK) k_po_scan_heads(unsigned* __restrict__ heads, unsigned n_tiles,
                                                                    unsigned long long* __restrict__ n_unique) {
    __shared__ unsigned ws[PO_WAVES];
    unsigned carry = 0;
#pragma unroll 1
    for (unsigned base = 0; base < n_tiles; base += PAIRS_SCAN_BLOCK) {
        const unsigned t = base + threadIdx.x;
        const unsigned v = t < n_tiles ? heads[t] : 0u;
        unsigned total;
        const unsigned before = trip_exclusive(v, ws, total);
        if (t < n_tiles) heads[t] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *n_unique = carry;
}

__global__ void __launch_bounds__(PAIRS_BLOCK) k_po_compact(const uint4* __restrict__ recs0, const uint4* __restrict__ recs1,
                                                            const unsigned* __restrict__ ctl, uint32_t k, const unsigned* __restrict__ heads,
                                                            uint32_t* __restrict__ tree_ids_out, uint64_t* __restrict__ leaf_ids_out,
                                                            uint32_t* __restrict__ indices_out, uint32_t* __restrict__ first) {
    __shared__ unsigned ws[PO_WAVES];
    const uint4* __restrict__ recs = ctl[PO_FINAL] ? recs1 : recs0;
    const size_t start = (size_t)blockIdx.x * PAIRS_TILE + threadIdx.x;
    unsigned placed = heads[blockIdx.x];
#pragma unroll 1
    for (unsigned r = 0; r < PAIRS_ROUNDS; ++r) {
        const size_t i = start + (size_t)r * PAIRS_BLOCK;
        const bool valid = i < k;
        const uint4 rec = valid ? recs[i] : make_uint4(0u, 0u, 0u, 0u);
        const bool head = valid && is_head(recs, i, rec);
        const unsigned long long mask = __ballot(head);
        unsigned total;
        const unsigned at = placed + waves_before(__popcll(mask), ws, total) + __popcll(mask & lanes_below());
        if (head && at < k) {
            if (tree_ids_out) tree_ids_out[at] = rec.x;
            if (leaf_ids_out) leaf_ids_out[at] = (uint64_t)rec.z | ((uint64_t)rec.w << 32);
            if (indices_out) indices_out[at] = rec.z;
            if (first) first[at] = rec.y;
        }
        placed += total;
    }
}

// ---- the launchers ----
namespace {

// the sort of the k pairs: into `order` when it is given, else as records in the array that ctl[PO_FINAL] names
hipError_t launch_sort(const void* tree_ids, const void* leaf_ids, size_t k, uint32_t* order, char* work, const PairsWork& w, hipStream_t st) {
    unsigned* ctl = reinterpret_cast<unsigned*>(work + w.ctl);
    unsigned* totals = reinterpret_cast<unsigned*>(work + w.totals);
    unsigned* counts = reinterpret_cast<unsigned*>(work + w.counts);
    uint4* recs[2] = {reinterpret_cast<uint4*>(work + w.recs[0]), reinterpret_cast<uint4*>(work + w.recs[1])};
    const uint32_t k32 = (uint32_t)k;
    const unsigned n_tiles = (unsigned)w.n_tiles;
    const dim3 blk(PAIRS_BLOCK), per_pair((unsigned)((k + PAIRS_BLOCK - 1) / PAIRS_BLOCK)), per_tile(n_tiles);
    hipError_t e = hipMemsetAsync(ctl, 0, PO_CTL_BYTES, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_po_load, per_pair, blk, 0, st, static_cast<const uint32_t*>(tree_ids), static_cast<const uint64_t*>(leaf_ids), k32,
                       recs[0], ctl);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_po_plan, dim3(1), dim3(64), 0, st, ctl);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (unsigned pass = 0; pass < PAIRS_PASSES; ++pass) {
        hipLaunchKernelGGL(k_po_count, per_tile, blk, 0, st, recs[0], recs[1], ctl, pass, k32, counts, n_tiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_po_scan, dim3(PAIRS_DIGITS), dim3(PAIRS_SCAN_BLOCK), 0, st, ctl, pass, counts, n_tiles, totals);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_po_scatter, per_tile, blk, 0, st, recs[0], recs[1], ctl, pass, k32, counts, n_tiles, totals, order);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_pairs_order(const void* tree_ids, const void* leaf_ids, size_t k, void* order, void* work, hipStream_t st) {
    return launch_sort(tree_ids, leaf_ids, k, static_cast<uint32_t*>(order), static_cast<char*>(work), pairs_work(k), st);
}

hipError_t launch_pairs_unique(const void* tree_ids, const void* leaf_ids, size_t k, void* tree_ids_out, void* leaf_ids_out, void* indices_out,
                               void* first, void* n_unique, void* work_, hipStream_t st) {
    char* work = static_cast<char*>(work_);
    const PairsWork w = pairs_work(k);
    hipError_t e = launch_sort(tree_ids, leaf_ids, k, nullptr, work, w, st);
    if (e != hipSuccess) return e;
    const unsigned* ctl = reinterpret_cast<const unsigned*>(work + w.ctl);
    unsigned* heads = reinterpret_cast<unsigned*>(work + w.counts);  // (the digit counts are done with)
    const uint4* recs[2] = {reinterpret_cast<const uint4*>(work + w.recs[0]), reinterpret_cast<const uint4*>(work + w.recs[1])};
    const uint32_t k32 = (uint32_t)k;
    const unsigned n_tiles = (unsigned)w.n_tiles;
    const dim3 blk(PAIRS_BLOCK), per_tile(n_tiles);
    hipLaunchKernelGGL(k_po_heads, per_tile, blk, 0, st, recs[0], recs[1], ctl, k32, heads);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_po_scan_heads, dim3(1), dim3(PAIRS_SCAN_BLOCK), 0, st, heads, n_tiles, static_cast<unsigned long long*>(n_unique));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_po_compact, per_tile, blk, 0, st, recs[0], recs[1], ctl, k32, heads, static_cast<uint32_t*>(tree_ids_out),
                       static_cast<uint64_t*>(leaf_ids_out), static_cast<uint32_t*>(indices_out), static_cast<uint32_t*>(first));
    return hipGetLastError();
}

}  // namespace p252
