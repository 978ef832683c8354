// forest_openings.hip — the openings half of the ragged forest (forest_ragged.hip): from a forest of trees of DIFFERENT sizes,
// built once with tree-major levels, k openings (tree id, leaf id) in one call, their re-hash with a depth per opening, and the
// comparison of each recomputed root with the root of ITS tree.  Opening i of tree t has depth_i = depth(n_t) levels; all
// arrays use one stride D = depth(max_leaves): leaves[k], siblings[k][D][arity - 1], positions[k][D], depths[k].
//
// Extraction (no hashing, HBM-bound byte movement):
//   k_fo_record      one lane per opening: the tree's record out of the forest's index (leaf start offsets[t], n_t, block start
//                    LO[t] — launch_forest_ragged_index, the build's own validation and scans), the leaf id, the depth byte;
//                    a bad opening (tree id >= n_trees, a bad tree, leaf id >= n_t) gets n = 0, depth 0xFF, one count
//   k_fr_openings    the scheme of k_merkle4_openings (openings.hip): six lanes per (opening, level), one per 16-byte piece of
//                    the 96-byte sibling record (arity 2: two lanes), lane t stores the t-th 16-byte word of the siblings array.
//                    The lane reads its opening's 32-byte record (one line serves the 6 D lanes of two openings) and finds its
//                    level's start inside the tree's block with the closed form of forest_ragged.hip (at most l - 1 additions);
//                    the per-block LDS table of openings.hip does not carry over, n_t differs per opening.  Rows l >= depth_i
//                    are written as zero.
// Re-hash:
//   a wave runs to its deepest lane, so the openings are sorted by depth, deepest first — a counting sort with one bin per
//   depth (k_fo_depth_hist: bins in LDS per tile of 2,048, one global atomic per non-empty bin; k_fo_depth_scan: one block;
//   k_fo_depth_scatter); bad depths sort last.  P252_RAGGED_SORT=0 (ragged.h) leaves the identity order.
//   k_path_ragged    lane j walks opening order[j] for its own depth and stores root order[j]: the child select of
//                    merkle4_path_body / k_merkle2_path around the library's permutation (hades_permute<0x02u, true> with the
//                    hoisted tag S-box), 3 waves per SIMD.  One fetch scheme: record by record (the whole-line scheme of
//                    k_merkle4_path_lines needs a wave-uniform level phase; the kernel is multiply-add-bound).
//   k_compare_roots_gather   ok[i] from roots[i] against expected[tree_ids[i]]
// ceil_shift, u64_of and the tree lookup are forest_node.hpp's.  k_fr_openings' level start, k_fo_record's depth and load_or_zero
// (openings.hip's) stay written out here: profiles/forest_kernels_refactor.txt has the reasons.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "fastdiv.hpp"
#include "forest_node.hpp"
#include "forest_openings.h"
#include "hades29.hpp"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FO_BLOCK = 256;
constexpr unsigned FO_ITEMS = 8;  // openings per thread of a sort block
constexpr unsigned FO_TILE = FO_BLOCK * FO_ITEMS;  // (the tile of bucket_hist / bucket_scatter, blockops.hpp)
constexpr unsigned FO_BAD_BIN = FOREST_OPENINGS_BINS - 1;

// a value select, not a pointer select (openings.hip: the pointer-select form parks the zero in scratch); word 0 of `base` exists
__device__ __forceinline__ uint4 load_or_zero(const uint4* __restrict__ base, size_t word, bool ok) {
    uint4 v = base[ok ? word : 0];
    v.x = ok ? v.x : 0u;
    v.y = ok ? v.y : 0u;
    v.z = ok ? v.z : 0u;
    v.w = ok ? v.w : 0u;
    return v;
}

}  // namespace

// ---- the record of each opening: {leaf start of the tree, n_t (0: bad), LO[t], leaf id} as two 16-byte words ----
__global__ void __launch_bounds__(FO_BLOCK) k_fo_record(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                        const uint64_t* __restrict__ LO, size_t n_trees,
                                                        const uint32_t* __restrict__ tree_ids, const uint64_t* __restrict__ leaf_ids,
                                                        size_t k, unsigned la, uint4* __restrict__ rec, uint8_t* __restrict__ depths,
                                                        unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * FO_BLOCK + threadIdx.x;
    if (i >= k) return;
    const size_t t = tree_ids[i];
    const uint64_t leaf = leaf_ids[i];
    size_t ts;
    const uint64_t n = forest_tree_leaves(ntree, n_trees, t, &ts);
    const bool good = n != 0 && leaf < n;
    const uint64_t leaf0 = good ? offsets[ts] : 0ull, lo = good ? LO[ts] : 0ull, nn = good ? n : 0ull, lf = good ? leaf : 0ull;
    unsigned d = 0;  // p252_merkle{4,2}_depth(nn)
#pragma unroll 1
    for (uint64_t c = nn; c > 1; c = ceil_shift(c, la)) ++d;
    rec[2 * i] = make_uint4((unsigned)leaf0, (unsigned)(leaf0 >> 32), (unsigned)nn, (unsigned)(nn >> 32));
    rec[2 * i + 1] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)lf, (unsigned)(lf >> 32));
    depths[i] = good ? (uint8_t)d : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
    if (!good && n_bad) atomicAdd(n_bad, 1u);
}

// ---- the pieces.  IDX = uint32_t whenever the launch has fewer than 2^32 lanes (the opening and the level then come from the
// reciprocal product of fastdiv.hpp), size_t otherwise.  D == 0 (every tree a single leaf): two lanes per opening copy the leaf. ----
template <class IDX, unsigned ARITY>
__global__ void __launch_bounds__(FO_BLOCK) k_fr_openings(const uint4* __restrict__ leaves, const uint4* __restrict__ levels,
                                                          const uint4* __restrict__ rec, size_t k, unsigned D, unsigned long long inv_D,
                                                          uint4* __restrict__ leaves_out, uint4* __restrict__ siblings,
                                                          uint8_t* __restrict__ positions) {
    const IDX t = (IDX)blockIdx.x * FO_BLOCK + threadIdx.x;  // = the index of the 16-byte word of `siblings` this lane stores
    if (D == 0) {
        if (t >= 2 * k) return;
        const size_t i = t >> 1;
        const uint4 r0 = rec[2 * i], r1 = rec[2 * i + 1];
        const uint64_t leaf0 = u64_of(r0.x, r0.y), n = u64_of(r0.z, r0.w), leaf = u64_of(r1.z, r1.w);
        leaves_out[t] = load_or_zero(leaves, 2 * (size_t)(leaf0 + leaf) + (t & 1), n != 0);
        return;
    }
    constexpr unsigned PIECES = 2 * (ARITY - 1), SHIFT = ARITY == 4 ? 2 : 1;
    if (t >= (IDX)(k * D * PIECES)) return;
    const IDX r = t / PIECES;  // the (opening, level) row
    const unsigned piece = (unsigned)(t - r * PIECES), sib = piece >> 1, half = piece & 1u;
    const IDX i = sizeof(IDX) == 4 ? (IDX)fast_div((unsigned)r, inv_D) : r / (IDX)D;
    const unsigned l = (unsigned)(r - i * D);
    const uint4 r0 = rec[2 * (size_t)i], r1 = rec[2 * (size_t)i + 1];
    const uint64_t leaf0 = u64_of(r0.x, r0.y), n = u64_of(r0.z, r0.w), lo = u64_of(r1.x, r1.y), leaf = u64_of(r1.z, r1.w);
    const bool good = n != 0;
    if (l == 0 && piece < 2) leaves_out[2 * (size_t)i + piece] = load_or_zero(leaves, 2 * (size_t)(leaf0 + leaf) + piece, good);
    // level l of the tree (level 0 = its leaves) has cnt nodes; the opening has a row l while that level has more than one
    const uint64_t cnt = ceil_shift(n, l * SHIFT);
    const bool live = good && cnt > 1;
    uint64_t first = l == 0 ? leaf0 : lo;  // the level's first node, in scalars of its array: lo + level_start(n, l, SHIFT), written out
#pragma unroll 1
    for (unsigned j = 1; j < l; ++j) first += ceil_shift(n, j * SHIFT);  // (levels 1 .. l-1 of the block before it)
    const uint64_t node = leaf >> (SHIFT * l);  // (l < D <= 64 / SHIFT)
    const unsigned p = (unsigned)(node & (ARITY - 1));
    const uint64_t j = node - p + sib + (sib >= p ? 1u : 0u);  // the group's nodes in order, the path's own node left out
    const bool ok = live && j < cnt;  // a ragged level's missing siblings are the zero scalar
    const uint4* nodes = (l == 0 || !ok) ? leaves : levels;
    siblings[t] = load_or_zero(nodes, 2 * (size_t)(first + j) + half, ok);
    if (piece == 0) positions[r] = live ? (uint8_t)p : (uint8_t)0;
}

// ---- the depth sort ----
__device__ __forceinline__ unsigned depth_bin(const uint8_t* __restrict__ depths, size_t i, unsigned stride) {
    const unsigned d = depths[i];
    return d <= stride ? d : FO_BAD_BIN;
}

__global__ void __launch_bounds__(FO_BLOCK) k_fo_depth_hist(const uint8_t* __restrict__ depths, size_t k, unsigned stride,
                                                            unsigned long long* __restrict__ hist) {
    bucket_hist<FO_BLOCK, FO_ITEMS, FOREST_OPENINGS_BINS>(k, hist, [=](size_t i) { return depth_bin(depths, i, stride); });
}

// counts -> the start of each bin in the sorted order: deepest first, the bad ones last; in place
__global__ void __launch_bounds__(64) k_fo_depth_scan(unsigned long long* __restrict__ hist) {
    if (threadIdx.x != 0) return;
    unsigned long long run = 0;
#pragma unroll 1
    for (int b = (int)FOREST_OPENINGS_MAX_DEPTH; b >= 0; --b) {
        const unsigned long long c = hist[b];
        hist[b] = run;
        run += c;
    }
    hist[FO_BAD_BIN] = run;
}

__global__ void __launch_bounds__(FO_BLOCK) k_fo_depth_scatter(const uint8_t* __restrict__ depths, size_t k, unsigned stride,
                                                               unsigned long long* __restrict__ cursor, uint64_t* __restrict__ order) {
    bucket_scatter<FO_BLOCK, FO_ITEMS, FOREST_OPENINGS_BINS>(k, cursor, order, [=](size_t i) { return depth_bin(depths, i, stride); });
}

// ---- the re-hash, one lane per opening: lane j walks opening order[j] (order == null: opening j) for depths[] levels ----
template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_path_ragged(const int32_t* __restrict__ tab, TagArg tag, const Scalar32* __restrict__ leaves, const Scalar32* __restrict__ siblings,
              const uint8_t* __restrict__ positions, const uint8_t* __restrict__ depths, unsigned stride,
              const uint64_t* __restrict__ order, Scalar32* __restrict__ roots, size_t k, unsigned* __restrict__ n_bad) {
    const size_t lane = (size_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (lane >= k) return;
    const size_t i = order ? (size_t)order[lane] : lane;
    if (i >= k) return;  // (order is the sort's own permutation of 0 .. k-1)
    const unsigned depth = depths[i];
    if (depth > stride) {  // a bad opening (0xFF) or a depth the layout cannot hold
        store_zero(roots + i);
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    E29 cur = load_scalar(leaves + i);
    const Scalar32* sib = siblings + i * stride * (ARITY - 1);
    const uint8_t* pos = positions + i * stride;
#pragma unroll 1
    for (unsigned l = 0; l < depth; ++l) {
        E29 s[WIDTH];
#pragma unroll
        for (int q = 0; q < NL; ++q) s[0].d[q] = tag.x0[q];  // lane 0 enters after its first S-box (hades_permute PRE0)
        if (ARITY == 4) {
            const unsigned p = pos[l] & 3u;
            const E29 a = load_scalar(sib + l * 3 + 0), b = load_scalar(sib + l * 3 + 1), c = load_scalar(sib + l * 3 + 2);
            // children = siblings with `cur` inserted at slot p (per-lane select, no divergence)
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                s[1].d[q] = p == 0 ? cur.d[q] : a.d[q];
                s[2].d[q] = p == 1 ? cur.d[q] : (p < 1 ? a.d[q] : b.d[q]);
                s[3].d[q] = p == 2 ? cur.d[q] : (p < 2 ? b.d[q] : c.d[q]);
                s[4].d[q] = p == 3 ? cur.d[q] : c.d[q];
            }
        } else {
            const bool right = (pos[l] & 1u) != 0;  // the path's node is the RIGHT child
            const E29 other = load_scalar(sib + l);
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                s[1].d[q] = right ? other.d[q] : cur.d[q];
                s[2].d[q] = right ? cur.d[q] : other.d[q];
            }
            s[3] = e29_zero();
            s[4] = e29_zero();
        }
        hades_permute<0x02u, true>(s, tab);  // only lane 1 is squeezed
        cur = s[1];
    }
    store_scalar(roots + i, cur);
}

// ---- a root per opening: ok[i] = 1 iff opening i is well-formed and re-hashed to the root of ITS tree ----
__global__ void __launch_bounds__(FO_BLOCK) k_compare_roots_gather(const uint4* __restrict__ roots, const uint8_t* __restrict__ depths,
                                                                   unsigned stride, const uint32_t* __restrict__ tree_ids,
                                                                   const uint4* __restrict__ expected, size_t n_trees,
                                                                   uint8_t* __restrict__ ok, size_t k) {
    const size_t i = (size_t)blockIdx.x * FO_BLOCK + threadIdx.x;
    if (i >= k) return;
    const size_t t = tree_ids[i];
    bool same = depths[i] <= stride && t < n_trees;
    if (same) {
        const uint4 e0 = expected[2 * t], e1 = expected[2 * t + 1], a = roots[2 * i], b = roots[2 * i + 1];
        same = a.x == e0.x && a.y == e0.y && a.z == e0.z && a.w == e0.w && b.x == e1.x && b.y == e1.y && b.z == e1.z && b.w == e1.w;
    }
    ok[i] = same ? (uint8_t)1 : (uint8_t)0;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
template <unsigned ARITY>
static hipError_t launch_pieces(const void* leaves, const void* levels, const void* records, size_t k, unsigned D, void* leaves_out,
                                void* siblings, void* positions, hipStream_t st) {
    if (k == 0) return hipSuccess;
    const size_t lanes = D ? k * D * 2 * (ARITY - 1) : 2 * k;
    const dim3 grid((unsigned)((lanes + FO_BLOCK - 1) / FO_BLOCK));
    const unsigned long long inv_D = fast_div_reciprocal(D);
    if (lanes + FO_BLOCK <= 0xffffffffull)
        hipLaunchKernelGGL((k_fr_openings<uint32_t, ARITY>), grid, dim3(FO_BLOCK), 0, st, static_cast<const uint4*>(leaves),
                           static_cast<const uint4*>(levels), static_cast<const uint4*>(records), k, D, inv_D, static_cast<uint4*>(leaves_out),
                           static_cast<uint4*>(siblings), static_cast<uint8_t*>(positions));
    else
        hipLaunchKernelGGL((k_fr_openings<size_t, ARITY>), grid, dim3(FO_BLOCK), 0, st, static_cast<const uint4*>(leaves),
                           static_cast<const uint4*>(levels), static_cast<const uint4*>(records), k, D, inv_D, static_cast<uint4*>(leaves_out),
                           static_cast<uint4*>(siblings), static_cast<uint8_t*>(positions));
    return hipGetLastError();
}

hipError_t launch_forest_openings(unsigned arity, const void* leaves, const void* levels, const void* offsets, const uint64_t* ntree,
                                  const uint64_t* lo, size_t n_trees, const void* tree_ids, const void* leaf_ids, size_t k,
                                  unsigned stride_depth, void* records, void* leaves_out, void* siblings, void* positions, void* depths,
                                  void* n_bad, hipStream_t st) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fo_record, dim3((unsigned)((k + FO_BLOCK - 1) / FO_BLOCK)), dim3(FO_BLOCK), 0, st,
                       static_cast<const uint64_t*>(offsets), ntree, lo, n_trees, static_cast<const uint32_t*>(tree_ids),
                       static_cast<const uint64_t*>(leaf_ids), k, arity == 4 ? 2u : 1u, static_cast<uint4*>(records),
                       static_cast<uint8_t*>(depths), static_cast<unsigned*>(n_bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_forest_opening_pieces(arity, leaves, levels, records, k, stride_depth, leaves_out, siblings, positions, st);
}

hipError_t launch_forest_opening_pieces(unsigned arity, const void* leaves, const void* levels, const void* records, size_t k,
                                        unsigned stride_depth, void* leaves_out, void* siblings, void* positions, hipStream_t st) {
    return arity == 4 ? launch_pieces<4>(leaves, levels, records, k, stride_depth, leaves_out, siblings, positions, st)
                      : launch_pieces<2>(leaves, levels, records, k, stride_depth, leaves_out, siblings, positions, st);
}

hipError_t launch_forest_depth_sort(const void* depths, size_t k, unsigned stride_depth, void* order, void* hist, hipStream_t st) {
    if (k == 0) return hipSuccess;
    const uint8_t* dp = static_cast<const uint8_t*>(depths);
    unsigned long long* h = static_cast<unsigned long long*>(hist);
    const unsigned tiles = (unsigned)((k + FO_TILE - 1) / FO_TILE);
    const hipError_t e = hipMemsetAsync(hist, 0, forest_openings_hist_bytes(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fo_depth_hist, dim3(tiles), dim3(FO_BLOCK), 0, st, dp, k, stride_depth, h);
    hipLaunchKernelGGL(k_fo_depth_scan, dim3(1), dim3(64), 0, st, h);
    hipLaunchKernelGGL(k_fo_depth_scatter, dim3(tiles), dim3(FO_BLOCK), 0, st, dp, k, stride_depth, h, static_cast<uint64_t*>(order));
    return hipGetLastError();
}

hipError_t launch_path_ragged(unsigned arity, const int32_t* tab, const TagArg& tag, const void* leaves, const void* siblings,
                              const void* positions, const void* depths, unsigned stride_depth, void* roots, size_t k, void* n_bad,
                              void* order, void* hist, hipStream_t st) {
    if (k == 0) return hipSuccess;
    const uint8_t* dp = static_cast<const uint8_t*>(depths);
    const uint64_t* ord = nullptr;
    if (order && hist) {
        const hipError_t e = launch_forest_depth_sort(depths, k, stride_depth, order, hist, st);
        if (e != hipSuccess) return e;
        ord = static_cast<const uint64_t*>(order);
    }
    // (small k runs the one-lane kernel too: no lane-group re-hash here)
    auto kern = arity == 4 ? k_path_ragged<4> : k_path_ragged<2>;
    return launch(kern, k, st, tab, tag, static_cast<const Scalar32*>(leaves), static_cast<const Scalar32*>(siblings),
                  static_cast<const uint8_t*>(positions), dp, stride_depth, ord, static_cast<Scalar32*>(roots), k,
                  static_cast<unsigned*>(n_bad));
}

hipError_t launch_compare_roots_gather(const void* roots, const void* depths, unsigned stride_depth, const void* tree_ids,
                                       const void* expected, size_t n_trees, void* ok, size_t k, hipStream_t st) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_compare_roots_gather, dim3((unsigned)((k + FO_BLOCK - 1) / FO_BLOCK)), dim3(FO_BLOCK), 0, st,
                       static_cast<const uint4*>(roots), static_cast<const uint8_t*>(depths), stride_depth,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint4*>(expected), n_trees, static_cast<uint8_t*>(ok), k);
    return hipGetLastError();
}

}  // namespace p252
