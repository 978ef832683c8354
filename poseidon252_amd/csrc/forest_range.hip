// forest_range.hip — m RUNS of leaves of the trees of a ragged forest (forest_ragged.hip) proved and checked in one call, for both
// arities.  Run r is leaves [a, b) of tree t, b = a + len; its leaves sit at leaf_offsets[r] of a flat array, the layout of the ragged
// calls.  With a_l = floor(a / A^l), b_l = ceil(b / A^l) and w_l = ceil(n_t / A^l) the nodes of level l that a verifier knows or
// computes are the interval [a_l, b_l), and the proof of level l is the nodes [A a_{l+1}, a_l) left of it, then
// [b_l, min(A b_{l+1}, w_l)) right of it: at most 2 (A - 1) scalars a level, byte for byte what multiproof.hip writes for the
// positions a .. b - 1.  Nothing here needs a structure pass: every place is a closed form of (n_t, a, b).
//   (launch_forest_ragged_index over d_leaf_offsets: the runs' lengths by the ragged forest's own rule, 0 for bad offsets)
//   k_rg_check       one lane per run: its tree's leaf count (the forest's index, or the verifier's claimed count), the bad-run
//                    rule, the closed-form proof length; n[r] (0: nothing of run r is read or hashed) for every later kernel.
//                    Extraction's lengths and counts, and the count of bad runs, are written here.
//   k_rg_gather      extraction: one lane per scalar of a proof row — (run, level, sibling slot) found by walking the run's levels —
//                    moves 32 bytes with two 16-byte accesses, or writes the row's zero tail
//   (launch_forest_scan_rows: cnt[l][r] = b_l - a_l of the good runs, which k_rg_check wrote, scanned over the runs for every level
//                    at once by the ragged forest's own three-pass scan: base[l][r] = the place of run r's first node in the DENSE
//                    list of level l, ctr[l] = the list's length.  No idle slot is ever hashed.)
//   k_rg_move        extraction: one lane per 16-byte half of a leaf of the dense level 0, its run by binary search in base[0]:
//                    the relocation is balanced over scalars, not over runs (as the select's k_fr_sel_move)
//   k_rg_records     verification, level l -> l + 1: one lane per node of the dense list of level l + 1, its run by binary search in
//                    base[l + 1]; writes the 16-byte record of multiproof.hip (parent, start of its children's run in the value
//                    list below — the caller's leaves for l = 0 —, proof offset, mask of the child slots inside [a_l, b_l)) and the
//                    width w_l.  The same launch deposits the value of every run whose tree ends at level l: its root.
//   k_rg_leaf_roots  one lane per run: a one-leaf tree's root, its leaf mod p (the forest's convention), deposited like the others
//   k_rg_finish      one lane per run: the verdict byte, the recomputed root, the digest count
// The digests run through launch_multiproof_digest_list (multiproof.hip's k_mp_digest / k_mp_digest_coop on this unit's records): no
// kernel here runs the permutation.  ceil_shift, u64_of and words_mod_p are forest_node.hpp's; the scans are forest_ragged.hip's.
#include <hip/hip_runtime.h>

#include "forest_node.hpp"
#include "forest_ragged.h"
#include "forest_range.h"
#include "multiproof.h"

namespace p252 {

namespace {

constexpr unsigned RG_BLOCK = 256;       // threads of a block
constexpr size_t RG_COUNT_BYTES = 1024;  // ctr[l] = nodes of the dense level l, l = 0 .. 32 (uint64 words)
constexpr unsigned RG_MASK_SHIFT = 28;   // a record's last word: proof offset bits 32 .. 59, slot mask above (multiproof.hip's)
constexpr uint32_t RG_BAD_LEN = 0xffffffffu;

typedef unsigned long long u64;

// level l of run [a, b) of a tree of n leaves.  A good run has a < b <= n <= max_leaves < 2^32: 32-bit words hold every node index
struct RgLevel {
    uint32_t a, b, w;      // the interval [a_l, b_l) and the level's width
    unsigned left, right;  // proof nodes left and right of the interval
};
__device__ __forceinline__ uint32_t shr32(uint32_t v, unsigned k) { return k >= 32 ? 0u : v >> k; }
__device__ __forceinline__ uint32_t ceil_shift32(uint32_t v, unsigned k) {
    return k >= 32 ? (uint32_t)(v != 0) : (v >> k) + ((v & ((1u << k) - 1u)) != 0);
}
template <unsigned ARITY>
__device__ __forceinline__ RgLevel rg_level(uint32_t n, uint32_t a, uint32_t b, unsigned l) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    const unsigned sh = l * LA;
    RgLevel v;
    v.a = shr32(a, sh);
    v.b = ceil_shift32(b, sh);
    v.w = ceil_shift32(n, sh);
    v.left = v.a & (ARITY - 1);  // a_l - A a_{l+1}
    const unsigned fill = (ARITY - (v.b & (ARITY - 1))) & (ARITY - 1);  // A b_{l+1} - b_l: to the end of the last parent's children
    const uint32_t room = v.w - v.b;
    v.right = fill < room ? fill : room;  // min(A b_{l+1}, w_l) - b_l
    return v;
}

// nodes of run [a, b) on level l of a tree of n leaves (n == 0: not a good run; 0 as well above the tree's root)
__device__ __forceinline__ uint64_t rg_count(uint64_t n, uint64_t a, uint64_t b, unsigned l, unsigned la) {
    if (n == 0 || (l > 0 && ceil_shift(n, (l - 1) * la) <= 1)) return 0;
    return ceil_shift(b, l * la) - (a >> (l * la));
}

// the run that holds node g of a dense list: the largest r in [0, m) with row[r] <= g (row ascending, row[0] = 0 <= g) — of runs that
// start at the same place the last, the one that has nodes
__device__ __forceinline__ size_t run_of(const uint64_t* __restrict__ row, size_t m, uint64_t g) {
    size_t lo = 0, hi = m - 1;
    while (lo < hi) {
        const size_t mid = (lo + hi + 1) >> 1;
        if (row[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

}  // namespace

// the m runs as the caller gave them, and what k_rg_check made of them
struct RgRuns {
    const uint32_t* tree_ids;
    const uint64_t* first;
    const uint64_t* leaf_offsets;
    const uint64_t* len;  // the index over leaf_offsets: 0 for bad offsets
    uint64_t* n;          // the tree's leaf count, 0 unless the run is good (verification: and its proof length is the closed form's)
    size_t m;
};

// ---- the runs themselves.  counts: the verifier's claimed count per RUN, or (extraction) the forest's index per TREE ----
template <unsigned ARITY>
__global__ void __launch_bounds__(RG_BLOCK) k_rg_check(RgRuns R, const uint64_t* __restrict__ counts, bool verify, size_t n_trees,
                                                       uint64_t max_leaves, const uint32_t* __restrict__ lens_in, uint64_t proof_stride,
                                                       uint32_t* __restrict__ lens_out, uint64_t* __restrict__ counts_out,
                                                       unsigned* __restrict__ n_bad, uint64_t* __restrict__ cnt, unsigned row0,
                                                       unsigned rows) {
    const size_t r = (size_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (r >= R.m) return;
    const uint64_t len = R.len[r], a = R.first[r];
    const size_t t = R.tree_ids[r];
    uint64_t n = 0;
    if (t < n_trees) n = verify ? counts[r] : counts[t];
    const bool good = len != 0 && n >= 1 && n <= max_leaves && a <= n && len <= n - a;  // (a + len <= n without the sum)
    uint64_t length = 0;
    if (good) {
#pragma unroll 1
        for (unsigned l = 0; ceil_shift(n, l * (ARITY == 4 ? 2 : 1)) > 1; ++l) {
            const RgLevel v = rg_level<ARITY>((uint32_t)n, (uint32_t)a, (uint32_t)(a + len), l);
            length += v.left + v.right;
        }
    }
    if (!good && n_bad) atomicAdd(n_bad, 1u);
    uint64_t take = good ? n : 0;  // what every later kernel asks
    if (verify) {
        if (lens_in[r] != length || length > proof_stride) take = 0;
    } else {
        lens_out[r] = good ? (uint32_t)length : RG_BAD_LEN;
        counts_out[r] = take;
    }
    R.n[r] = take;
    // the run's nodes on levels row0 .. row0 + rows - 1: the rows that launch_forest_scan_rows turns into the dense lists' bases
#pragma unroll 1
    for (unsigned l = row0; l < row0 + rows; ++l) cnt[(size_t)l * R.m + r] = rg_count(take, a, a + len, l, ARITY == 4 ? 2 : 1);
}

// ---- extraction: scalar q of row r of the proof (stride scalars a row) ----
template <unsigned ARITY>
__global__ void __launch_bounds__(RG_BLOCK) k_rg_gather(RgRuns R, size_t lanes, unsigned stride, const uint64_t* __restrict__ offsets,
                                                        const uint64_t* __restrict__ lo, const uint4* __restrict__ leaves,
                                                        const uint4* __restrict__ levels, uint4* __restrict__ proof) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    const uint64_t g = (uint64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    const size_t r = (size_t)(g / stride);
    unsigned q = (unsigned)(g - (uint64_t)r * stride);
    const uint32_t n = (uint32_t)R.n[r];
    uint4 lo4 = make_uint4(0u, 0u, 0u, 0u), hi4 = lo4;  // (a bad run's row, and a good row's tail: zero)
    if (n) {
        const size_t t = R.tree_ids[r];  // (a good run: t < n_trees)
        const uint32_t a = (uint32_t)R.first[r], b = a + (uint32_t)R.len[r];
        uint64_t start = 0;  // of level l >= 1 inside the tree's block of the levels
#pragma unroll 1
        for (unsigned l = 0; ceil_shift32(n, l * LA) > 1; ++l) {
            const RgLevel v = rg_level<ARITY>(n, a, b, l);
            if (q < v.left + v.right) {
                const uint32_t node = q < v.left ? v.a - v.left + q : v.b + (q - v.left);  // (< w_l: the closed form)
                const uint4* src = l == 0 ? leaves + 2 * (size_t)(offsets[t] + node) : levels + 2 * (size_t)(lo[t] + start + node);
                lo4 = src[0];
                hi4 = src[1];
                break;
            }
            q -= v.left + v.right;
            if (l > 0) start += v.w;
        }
    }
    proof[2 * g] = lo4;
    proof[2 * g + 1] = hi4;
}

// ---- extraction: the leaves of the good runs, balanced over the scalars of the dense level 0 ----
__global__ void __launch_bounds__(RG_BLOCK) k_rg_move(RgRuns R, const uint64_t* __restrict__ base0, const u64* __restrict__ ctr, size_t lanes,
                                                      const uint64_t* __restrict__ offsets, const uint4* __restrict__ leaves,
                                                      uint4* __restrict__ out) {
    const uint64_t h = (uint64_t)blockIdx.x * RG_BLOCK + threadIdx.x;  // the 16-byte half
    const uint64_t s = h >> 1;
    if (h >= lanes || s >= ctr[0]) return;
    const size_t r = run_of(base0, R.m, s);
    const uint64_t j = s - base0[r];                          // (< len: a good run, inside leaf_offsets[r + 1] <= k)
    const size_t from = (size_t)(offsets[R.tree_ids[r]] + R.first[r] + j);
    out[2 * (size_t)(R.leaf_offsets[r] + j) + (h & 1)] = leaves[2 * from + (h & 1)];
}

// ---- verification: the records of level l + 1, and the roots of the trees that end at level l ----
template <unsigned ARITY>
__global__ void __launch_bounds__(RG_BLOCK) k_rg_records(RgRuns R, const uint64_t* __restrict__ base, const u64* __restrict__ ctr, unsigned l,
                                                         size_t lanes, uint64_t proof_stride, uint4* __restrict__ rec,
                                                         uint32_t* __restrict__ wnode, size_t cap, const uint4* __restrict__ vals,
                                                         uint4* __restrict__ rootval) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    const uint64_t g = (uint64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (g >= lanes) return;
    if (l >= 1 && g < R.m) {  // (vals: the values of the dense level l)
        const uint64_t n = R.n[g];
        if (n && ceil_shift(n, l * LA) == 1 && ceil_shift(n, (l - 1) * LA) > 1) {
            const size_t at = (size_t)base[(size_t)l * R.m + g];
            rootval[2 * g] = vals[2 * at];
            rootval[2 * g + 1] = vals[2 * at + 1];
        }
    }
    if (g >= ctr[l + 1] || g >= cap) return;
    const uint64_t* __restrict__ row = base + (size_t)(l + 1) * R.m;
    const size_t r = run_of(row, R.m, g);
    const uint32_t n = (uint32_t)R.n[r], a = (uint32_t)R.first[r], b = a + (uint32_t)R.len[r];
    const uint32_t i = (uint32_t)(g - row[r]);
    const RgLevel v = rg_level<ARITY>(n, a, b, l);
    const uint32_t p = shr32(a, (l + 1) * LA) + i;  // the parent: node a_{l+1} + i of level l + 1
    // its children inside [a_l, b_l), as slots of the parent
    const unsigned s_lo = i == 0 ? v.left : 0u, s_hi = v.b - p * ARITY < ARITY ? v.b - p * ARITY : ARITY;  // (A p < b_l: the parent has a child there)
    const unsigned mask = ((1u << s_hi) - 1u) & ~((1u << s_lo) - 1u);
    const uint64_t run = (l == 0 ? R.leaf_offsets[r] : base[(size_t)l * R.m + r]) + (i == 0 ? 0u : p * ARITY - v.a);
    uint64_t off = (uint64_t)r * proof_stride;
#pragma unroll 1
    for (unsigned j = 0; j < l; ++j) {
        const RgLevel u = rg_level<ARITY>(n, a, b, j);
        off += u.left + u.right;
    }
    if (i > 0 && p + 1 == ceil_shift32(b, (l + 1) * LA)) off += v.left;  // the last parent, not also the first: past the left nodes
    rec[g] = make_uint4(p, (unsigned)run, (unsigned)off, ((unsigned)(off >> 32) & ((1u << RG_MASK_SHIFT) - 1)) | (mask << RG_MASK_SHIFT));
    wnode[g] = v.w;
}

// ---- verification: the forest's convention for a one-leaf tree — its root is its leaf mod p ----
__global__ void __launch_bounds__(RG_BLOCK) k_rg_leaf_roots(RgRuns R, const uint4* __restrict__ leaves_in, uint4* __restrict__ rootval) {
    const size_t r = (size_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (r >= R.m || R.n[r] != 1) return;
    const uint4* leaf = leaves_in + 2 * (size_t)R.leaf_offsets[r];
    uint4 lo = leaf[0], hi = leaf[1];
    words_mod_p(lo, hi);
    rootval[2 * r] = lo;
    rootval[2 * r + 1] = hi;
}

// ---- verification: one lane per run.  top: the values of the dense level `depth` ----
__global__ void __launch_bounds__(RG_BLOCK) k_rg_finish(RgRuns R, const uint64_t* __restrict__ base, const u64* __restrict__ ctr, unsigned depth,
                                                        unsigned la, const uint4* __restrict__ top, const uint4* __restrict__ rootval,
                                                        const uint4* __restrict__ roots, uint8_t* __restrict__ ok, uint4* __restrict__ roots_out, u64* __restrict__ n_hashed) {
    const size_t r = (size_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    if (r == 0 && n_hashed) {
        u64 hashed = 0;
        for (unsigned l = 1; l <= depth; ++l) hashed += ctr[l];
        *n_hashed = hashed;
    }
    if (r >= R.m) return;
    const uint64_t n = R.n[r];
    bool same = false;
    if (n) {
        // where the root is: k_rg_leaf_roots and k_rg_records deposited it, but for a tree that ends at the last level: its is in the last
        // value list
        const uint4* src = rootval + 2 * r;
        if (n > 1 && ceil_shift(n, (depth - 1) * la) > 1) src = top + 2 * (size_t)base[(size_t)depth * R.m + r];
        const uint4 lo = src[0], hi = src[1];
        if (roots_out) {
            roots_out[2 * r] = lo;
            roots_out[2 * r + 1] = hi;
        }
        const size_t t = R.tree_ids[r];  // (a good run: t < n_trees)
        const uint4 rlo = roots[2 * t], rhi = roots[2 * t + 1];
        same = lo.x == rlo.x && lo.y == rlo.y && lo.z == rlo.z && lo.w == rlo.w && hi.x == rhi.x && hi.y == rhi.y && hi.z == rhi.z &&
               hi.w == rhi.w;
    }
    ok[r] = same ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api_forest.cpp)
// ---------------------------------------------------------------------------------------------
namespace {

size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + RG_BLOCK - 1) / RG_BLOCK); }

// the scratch of one call, carved out of `work`: the runs' index first
struct RgWork {
    u64* ctr;
    uint64_t *n, *base, *tsum;
    uint4 *rootval, *rec;
    uint32_t* wnode;
};
RgWork rg_work(const ForestRangePlan& p, void* work, unsigned rows) {
    char* b = static_cast<char*>(work) + p.index_bytes;
    auto take = [&](size_t bytes) {
        char* at = b;
        b += round256(bytes);
        return at;
    };
    RgWork w;
    w.ctr = reinterpret_cast<u64*>(take(RG_COUNT_BYTES));
    w.n = reinterpret_cast<uint64_t*>(take(p.m * 8));
    w.base = reinterpret_cast<uint64_t*>(take((size_t)rows * p.m * 8));
    w.tsum = reinterpret_cast<uint64_t*>(take((size_t)rows * p.tiles * 8));
    w.rootval = reinterpret_cast<uint4*>(take(p.m * 32));  // (verification only, as the two below)
    w.rec = reinterpret_cast<uint4*>(take(p.bound[1] * 16));
    w.wnode = reinterpret_cast<uint32_t*>(take(p.bound[1] * 4));
    return w;
}

// the runs' index: the ragged forest's validation over leaf_offsets with k in the place of n_leaves (no run is longer than k)
hipError_t rg_index(const ForestRangePlan& p, const void* leaf_offsets, void* work, const uint64_t** len, hipStream_t st) {
    const uint64_t* unused = nullptr;
    return launch_forest_ragged_index(p.arity, leaf_offsets, p.m, p.k, p.k, work, len, &unused, st);
}

}  // namespace

size_t forest_range_stride(unsigned arity, size_t max_leaves) { return (size_t)2 * (arity - 1) * forest_ragged_depth(max_leaves, arity); }

ForestRangePlan forest_range_plan(unsigned arity, size_t max_leaves, size_t m, size_t k) {
    ForestRangePlan p;
    p.arity = arity;
    p.log2a = arity == 4 ? 2 : 1;
    p.m = m;
    p.k = k;
    p.max_leaves = max_leaves;
    if (m == 0 || k == 0 || max_leaves == 0) return p;
    p.depth = forest_ragged_depth(max_leaves, arity);
    if (p.depth > FOREST_RANGE_MAX_DEPTH) p.depth = FOREST_RANGE_MAX_DEPTH;  // (api_forest.cpp refuses max_leaves >= 2^32)
    p.tiles = forest_scan_rows_tiles(m);
    p.bound[0] = k;
    for (unsigned l = 1; l <= p.depth; ++l) {
        const size_t by_width = (k >> (l * p.log2a)) + 2 * m;
        p.bound[l] = k + m < by_width ? k + m : by_width;
    }
    p.index_bytes = forest_ragged_index_bytes(m);
    const size_t per_run = round256(RG_COUNT_BYTES) + round256(m * 8);
    p.extract_bytes = p.index_bytes + per_run + round256(m * 8) + round256(p.tiles * 8);
    const size_t rows = p.depth + 1;
    p.verify_bytes = p.index_bytes + per_run + round256(rows * m * 8) + round256(rows * p.tiles * 8) + round256(m * 32) +
                     round256(p.bound[1] * 16) + round256(p.bound[1] * 4);
    p.values_bytes = 2 * p.bound[1] * 32;
    return p;
}

hipError_t launch_forest_range_proofs(const ForestRangePlan& p, const void* leaves, const void* offsets, const void* levels,
                                      const uint64_t* ntree, const uint64_t* lo, size_t n_trees, const void* tree_ids, const void* first,
                                      const void* leaf_offsets, void* leaves_out, void* proof, void* proof_lens, void* counts_out,
                                      void* n_bad, void* work, hipStream_t st) {
    const RgWork w = rg_work(p, work, 1);
    RgRuns R;
    R.tree_ids = static_cast<const uint32_t*>(tree_ids);
    R.first = static_cast<const uint64_t*>(first);
    R.leaf_offsets = static_cast<const uint64_t*>(leaf_offsets);
    R.n = w.n;
    R.m = p.m;
    hipError_t e = rg_index(p, leaf_offsets, work, &R.len, st);
    if (e != hipSuccess) return e;
    const dim3 blk(RG_BLOCK), per_run(blocks_for(p.m));
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    const uint4* lv = static_cast<const uint4*>(leaves);
    const unsigned stride = (unsigned)forest_range_stride(p.arity, p.max_leaves);
    const size_t lanes = p.m * stride;
    if (p.arity == 4) {
        hipLaunchKernelGGL(k_rg_check<4>, per_run, blk, 0, st, R, ntree, false, n_trees, (uint64_t)p.max_leaves, (const uint32_t*)nullptr,
                           (uint64_t)0, static_cast<uint32_t*>(proof_lens), static_cast<uint64_t*>(counts_out), static_cast<unsigned*>(n_bad),
                           w.base, 0u, leaves_out ? 1u : 0u);
        if (lanes)
            hipLaunchKernelGGL(k_rg_gather<4>, dim3(blocks_for(lanes)), blk, 0, st, R, lanes, stride, off, lo, lv,
                               static_cast<const uint4*>(levels), static_cast<uint4*>(proof));
    } else {
        hipLaunchKernelGGL(k_rg_check<2>, per_run, blk, 0, st, R, ntree, false, n_trees, (uint64_t)p.max_leaves, (const uint32_t*)nullptr,
                           (uint64_t)0, static_cast<uint32_t*>(proof_lens), static_cast<uint64_t*>(counts_out), static_cast<unsigned*>(n_bad),
                           w.base, 0u, leaves_out ? 1u : 0u);
        if (lanes)
            hipLaunchKernelGGL(k_rg_gather<2>, dim3(blocks_for(lanes)), blk, 0, st, R, lanes, stride, off, lo, lv,
                               static_cast<const uint4*>(levels), static_cast<uint4*>(proof));
    }
    if (leaves_out) {
        const hipError_t e2 = launch_forest_scan_rows(w.base, 1, p.m, w.ctr, w.tsum, st);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(k_rg_move, dim3(blocks_for(2 * p.k)), blk, 0, st, R, w.base, w.ctr, 2 * p.k, off, lv, static_cast<uint4*>(leaves_out));
    }
    return hipGetLastError();
}

hipError_t launch_forest_range_verify(const int32_t* tab, const TagArg& tag, const ForestRangePlan& p, const void* tree_ids,
                                      const void* counts, const void* first, const void* leaf_offsets, const void* leaves_in,
                                      const void* proof, size_t proof_stride, const void* proof_lens, const void* roots, size_t n_trees,
                                      void* ok, void* roots_out, void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st) {
    const RgWork w = rg_work(p, work, p.depth + 1);
    RgRuns R;
    R.tree_ids = static_cast<const uint32_t*>(tree_ids);
    R.first = static_cast<const uint64_t*>(first);
    R.leaf_offsets = static_cast<const uint64_t*>(leaf_offsets);
    R.n = w.n;
    R.m = p.m;
    hipError_t e = rg_index(p, leaf_offsets, work, &R.len, st);
    if (e != hipSuccess) return e;
    const dim3 blk(RG_BLOCK), per_run(blocks_for(p.m));
    const uint64_t* cnt = static_cast<const uint64_t*>(counts);
    const uint32_t* lens = static_cast<const uint32_t*>(proof_lens);
    if (p.arity == 4)
        hipLaunchKernelGGL(k_rg_check<4>, per_run, blk, 0, st, R, cnt, true, n_trees, (uint64_t)p.max_leaves, lens, (uint64_t)proof_stride,
                           (uint32_t*)nullptr, (uint64_t*)nullptr, static_cast<unsigned*>(n_bad), w.base, 1u, p.depth);
    else
        hipLaunchKernelGGL(k_rg_check<2>, per_run, blk, 0, st, R, cnt, true, n_trees, (uint64_t)p.max_leaves, lens, (uint64_t)proof_stride,
                           (uint32_t*)nullptr, (uint64_t*)nullptr, static_cast<unsigned*>(n_bad), w.base, 1u, p.depth);
    hipLaunchKernelGGL(k_rg_leaf_roots, per_run, blk, 0, st, R, static_cast<const uint4*>(leaves_in), w.rootval);
    e = launch_forest_scan_rows(w.base + p.m, p.depth, p.m, w.ctr + 1, w.tsum, st);  // rows 1 .. depth
    Scalar32* vals[2] = {static_cast<Scalar32*>(values), static_cast<Scalar32*>(values) + p.bound[1]};
    for (unsigned l = 0; l < p.depth && e == hipSuccess; ++l) {
        const size_t lanes = p.bound[l + 1] > p.m ? p.bound[l + 1] : p.m;  // (the records; one lane per run for the roots)
        const uint4* below = reinterpret_cast<const uint4*>(vals[l & 1]);
        if (p.arity == 4)
            hipLaunchKernelGGL(k_rg_records<4>, dim3(blocks_for(lanes)), blk, 0, st, R, w.base, w.ctr, l, lanes, (uint64_t)proof_stride, w.rec,
                               w.wnode, p.bound[l + 1], below, w.rootval);
        else
            hipLaunchKernelGGL(k_rg_records<2>, dim3(blocks_for(lanes)), blk, 0, st, R, w.base, w.ctr, l, lanes, (uint64_t)proof_stride, w.rec,
                               w.wnode, p.bound[l + 1], below, w.rootval);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        MultiproofDigestList d;
        d.list = w.rec;
        d.count = w.ctr + (l + 1);
        d.vals_in = l == 0 ? leaves_in : static_cast<const void*>(vals[l & 1]);
        d.vals_out = vals[(l + 1) & 1];
        d.proof = proof;
        d.proof_len = p.m * proof_stride;
        d.w_node = w.wnode;
        d.bound = p.bound[l + 1];
        e = launch_multiproof_digest_list(tab, tag, p.arity, d, st);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rg_finish, per_run, blk, 0, st, R, w.base, w.ctr, p.depth, p.log2a, reinterpret_cast<const uint4*>(vals[p.depth & 1]),
                       w.rootval, static_cast<const uint4*>(roots), static_cast<uint8_t*>(ok),
                       static_cast<uint4*>(roots_out), static_cast<u64*>(n_hashed));
    return hipGetLastError();
}

}  // namespace p252
