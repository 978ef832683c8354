// forest_anchor.hip — roots and openings of the trees of a built ragged forest (forest_ragged.hip, tree-major levels) as they WERE at
// earlier leaf counts: the membership proof against an anchor, the root a tree had at count c <= n_t, with no second copy of the forest.
// With A = arity, f_l(c) = c / A^l and d_l(c) = f_l(c) % A, of the tree at c leaves:
//   node j of level l is the stored node while j < f_l(c) (it covers leaves below c only, and the tree only grew);
//   node j == f_l(c) exists iff c % A^l != 0 — the PARTIAL node P_l(c) = H(the stored nodes [A f_l(c), f_{l-1}(c)) of level l - 1, then
//   P_{l-1}(c) if it exists, then zeros): the carry of the consistency verifier's old chain (forest_consistency.hip);
//   nothing lies right of it; the root is P_depth(c)(c), or the stored node 0 of level depth(c) when c == A^depth(c).
// So an anchor costs depth(c) - l0 digests, l0 the lowest level whose digit of c is not zero, however many leaves are opened under it.
//
// The anchors (stage 1):
//   k_fa_anchor      one lane per anchor: its record {leaf start of the tree, c (0: bad), LO[t], n_t} out of the forest's index, the
//                    depth byte depth(c), the digest count; a bad anchor (tree id >= n_trees, a bad tree, c == 0, c > n_t) gets a
//                    zero root, depth 0xFF and one count
//   k_fa_children    level l = 1 .. D, one lane per 16-byte half of a child: anchor a's A children of P_l(c) — d_{l-1}(c) stored
//                    nodes (level 0: the tree's leaves, as their bytes; level >= 1: at LO[t] + level_start(n_t, l - 1), the GROWN
//                    tree's widths), then P_{l-1}(c) out of the table, then zeros — laid out as children[a][A]; all zero for an
//                    anchor that has no partial node on level l
//   (launch_merkle4 over those m nodes: P[l - 1][a].  No hashing kernel of this unit's own — every hashing kernel has its row in the
//    edge-value matrix of the tests — so the chains advance level by level through the library's digest launch, which also picks the
//    lane-group or the one-lane build by the batch size.  Anchors of one launch are all on the same level: chains of different
//    lengths cost no divergence, only idle digests of zero children for the anchors that have nothing on that level.)
//   k_fa_roots       one lane per valid anchor: P[depth(c) - 1][a], or the stored node / the single leaf, reduced as a one-leaf tree's
//                    root is
// The openings (stage 2, no hashing), the record-and-pieces pattern of forest_openings.hip:
//   k_fa_record      one lane per opening: {leaf start, n_t, LO[t], leaf id, c, anchor id}, c == 0 for a bad opening (anchor id >= m,
//                    a bad anchor, leaf id >= c), which gets depth 0xFF and one count
//   k_fa_openings    k_fr_openings with the cut-off: row l is live while l < depth(c); sibling j of level l is the stored node when
//                    j < f_l(c), P[l - 1][a] when j == f_l(c) and c % A^l != 0, zero otherwise.  At most one sibling of an opening is
//                    a partial node: above the lowest row where leaf and c share a group P_l(c) is the leaf's own ancestor.
#include <hip/hip_runtime.h>

#include "fastdiv.hpp"
#include "forest_anchor.h"
#include "forest_node.hpp"
#include "forest_openings.h"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FA_BLOCK = 256;

// c % 2^s for any s
__device__ __forceinline__ uint64_t low_bits(uint64_t c, unsigned s) { return s >= 64 ? c : c & ((1ull << s) - 1); }
// p252_merkle{4,2}_depth(c)
__device__ __forceinline__ unsigned depth_of(uint64_t c, unsigned la) {
    unsigned d = 0;
#pragma unroll 1
    for (uint64_t w = c; w > 1; w = ceil_shift(w, la)) ++d;
    return d;
}
// the lowest level whose digit of c is not zero; depth(c) when c is a power of the arity: nothing to hash
__device__ __forceinline__ unsigned lowest_digit(uint64_t c, unsigned dc, unsigned la) {
    unsigned l0 = 0;
#pragma unroll 1
    while (l0 < dc && ((c >> (la * l0)) & ((1u << la) - 1)) == 0) ++l0;
    return l0;
}

#define ZERO4 make_uint4(0u, 0u, 0u, 0u)

}  // namespace

// ---- the record of each anchor: {leaf start of the tree, c (0: bad)}, {LO[t], n_t} ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_anchor(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                        const uint64_t* __restrict__ LO, size_t n_trees,
                                                        const uint32_t* __restrict__ tree_ids, const uint64_t* __restrict__ counts, size_t m,
                                                        unsigned la, uint4* __restrict__ arec, Scalar32* __restrict__ roots,
                                                        uint8_t* __restrict__ depths, unsigned* __restrict__ n_bad,
                                                        unsigned long long* __restrict__ n_hashed) {
    __shared__ unsigned block_hashed;
    if (threadIdx.x == 0) block_hashed = 0;
    __syncthreads();
    const size_t a = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    unsigned hashed = 0;
    if (a < m) {
        const size_t t = tree_ids[a];
        const uint64_t c = counts[a];
        size_t ts;
        const uint64_t nt = forest_tree_leaves(ntree, n_trees, t, &ts);
        const bool good = nt != 0 && c >= 1 && c <= nt;
        const uint64_t leaf0 = good ? offsets[ts] : 0ull, lo = good ? LO[ts] : 0ull, cc = good ? c : 0ull, nn = good ? nt : 0ull;
        const unsigned dc = depth_of(cc, la);
        arec[2 * a] = make_uint4((unsigned)leaf0, (unsigned)(leaf0 >> 32), (unsigned)cc, (unsigned)(cc >> 32));
        arec[2 * a + 1] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)nn, (unsigned)(nn >> 32));
        depths[a] = good ? (uint8_t)dc : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
        if (good) {
            hashed = dc - lowest_digit(cc, dc, la);
        } else {
            store_zero(roots + a);
            if (n_bad) atomicAdd(n_bad, 1u);
        }
    }
    if (!n_hashed) return;  // (uniform)
    if (hashed) atomicAdd(&block_hashed, hashed);  // one global atomic per block
    __syncthreads();
    if (threadIdx.x == 0 && block_hashed) atomicAdd(n_hashed, (unsigned long long)block_hashed);
}

// ---- the children of every anchor's partial node of level l, as launch_merkle4 reads them: children[a][ARITY] ----
template <unsigned ARITY>
__global__ void __launch_bounds__(FA_BLOCK) k_fa_children(const uint4* __restrict__ leaves, const uint4* __restrict__ levels,
                                                          const uint4* __restrict__ arec, const uint4* __restrict__ partial, size_t m,
                                                          unsigned l, uint4* __restrict__ children) {
    constexpr unsigned SHIFT = ARITY == 4 ? 2 : 1, PIECES = 2 * ARITY;
    const size_t t = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;  // = the index of the 16-byte word of `children` this lane stores
    if (t >= m * PIECES) return;
    const size_t a = t / PIECES;
    const unsigned piece = (unsigned)(t - a * PIECES), child = piece >> 1, half = piece & 1u;
    const uint4 r0 = arec[2 * a], r1 = arec[2 * a + 1];
    const uint64_t leaf0 = u64_of(r0.x, r0.y), c = u64_of(r0.z, r0.w), lo = u64_of(r1.x, r1.y), nt = u64_of(r1.z, r1.w);
    const unsigned below = l - 1;  // the children's level (SHIFT * below < 64: l <= the stride)
    // P_l(c) exists iff c % A^l != 0, and level l belongs to the tree at c leaves while level l - 1 has more than one node
    const bool active = low_bits(c, SHIFT * l) != 0 && ceil_shift(c, SHIFT * below) > 1;
    const uint64_t fb = c >> (SHIFT * below);  // f_{l-1}(c): the final nodes of level l - 1
    const unsigned d = (unsigned)(fb & (ARITY - 1));
    uint4 v = ZERO4;
    if (active && child < d) {  // a stored node, final at count c (fb - d + child < fb <= the level's width at n_t)
        const uint64_t first = below == 0 ? leaf0 : lo + level_start(nt, below, SHIFT);
        v = (below == 0 ? leaves : levels)[2 * (size_t)(first + fb - d + child) + half];
    } else if (active && child == d && low_bits(c, SHIFT * below) != 0) {  // the carry P_{l-1}(c) (below >= 1: c % 1 == 0)
        v = partial[2 * ((size_t)(below - 1) * m + a) + half];
    }
    children[t] = v;
}

// ---- the roots of the valid anchors ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_roots(const Scalar32* __restrict__ leaves, const Scalar32* __restrict__ levels,
                                                       const uint4* __restrict__ arec, const uint4* __restrict__ partial, size_t m,
                                                       unsigned la, Scalar32* __restrict__ roots) {
    const size_t a = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    if (a >= m) return;
    const uint4 r0 = arec[2 * a], r1 = arec[2 * a + 1];
    const uint64_t leaf0 = u64_of(r0.x, r0.y), c = u64_of(r0.z, r0.w), lo = u64_of(r1.x, r1.y), nt = u64_of(r1.z, r1.w);
    if (c == 0) return;  // (a bad anchor: k_fa_anchor wrote its zero root)
    const unsigned dc = depth_of(c, la);
    if (dc > lowest_digit(c, dc, la)) {  // P_dc(c), as the digest launch stored it
        uint4* dst = reinterpret_cast<uint4*>(roots + a);
        dst[0] = partial[2 * ((size_t)(dc - 1) * m + a)];
        dst[1] = partial[2 * ((size_t)(dc - 1) * m + a) + 1];
        return;
    }
    // c == A^dc: the stored node 0 of level dc; c == 1: the leaf, REDUCED as the build writes a one-leaf tree's root (k_fr_prep)
    const Scalar32* src = dc == 0 ? leaves + leaf0 : levels + lo + level_start(nt, dc, la);
    store_scalar(roots + a, load_scalar(src));
}

// ---- the record of each opening: {leaf start, n_t}, {LO[t], leaf id}, {c (0: bad), anchor id} as three 16-byte words ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_record(const uint4* __restrict__ arec, size_t m, const uint32_t* __restrict__ anchor_ids,
                                                        const uint64_t* __restrict__ leaf_ids, size_t k, unsigned la,
                                                        uint4* __restrict__ rec, uint8_t* __restrict__ depths, unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    if (i >= k) return;
    const size_t a = anchor_ids[i];
    const uint64_t leaf = leaf_ids[i];
    uint4 r0 = ZERO4, r1 = ZERO4;
    if (a < m) {
        r0 = arec[2 * a];
        r1 = arec[2 * a + 1];
    }
    const uint64_t c = u64_of(r0.z, r0.w);
    const bool good = c != 0 && leaf < c;
    rec[3 * i] = good ? make_uint4(r0.x, r0.y, r1.z, r1.w) : ZERO4;
    rec[3 * i + 1] = good ? make_uint4(r1.x, r1.y, (unsigned)leaf, (unsigned)(leaf >> 32)) : ZERO4;
    rec[3 * i + 2] = good ? make_uint4(r0.z, r0.w, (unsigned)a, 0u) : ZERO4;
    depths[i] = good ? (uint8_t)depth_of(c, la) : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
    if (!good && n_bad) atomicAdd(n_bad, 1u);
}

// ---- the pieces: k_fr_openings' lanes (forest_openings.hip), one per 16-byte piece of a sibling row; IDX as there ----
template <class IDX, unsigned ARITY>
__global__ void __launch_bounds__(FA_BLOCK) k_fa_openings(const uint4* __restrict__ leaves, const uint4* __restrict__ levels,
                                                          const uint4* __restrict__ rec, const uint4* __restrict__ partial, size_t m,
                                                          size_t k, unsigned D, unsigned long long inv_D, uint4* __restrict__ leaves_out,
                                                          uint4* __restrict__ siblings, uint8_t* __restrict__ positions) {
    const IDX t = (IDX)blockIdx.x * FA_BLOCK + threadIdx.x;  // = the index of the 16-byte word of `siblings` this lane stores
    if (D == 0) {  // every anchor a single leaf: two lanes per opening copy it
        if (t >= 2 * k) return;
        const size_t i = t >> 1;
        const uint4 r0 = rec[3 * i], r1 = rec[3 * i + 1], r2 = rec[3 * i + 2];
        const bool good = u64_of(r2.x, r2.y) != 0;
        leaves_out[t] = good ? leaves[2 * (size_t)(u64_of(r0.x, r0.y) + u64_of(r1.z, r1.w)) + (t & 1)] : ZERO4;
        return;
    }
    constexpr unsigned PIECES = 2 * (ARITY - 1), SHIFT = ARITY == 4 ? 2 : 1;
    if (t >= (IDX)(k * D * PIECES)) return;
    const IDX r = t / PIECES;  // the (opening, level) row
    const unsigned piece = (unsigned)(t - r * PIECES), sib = piece >> 1, half = piece & 1u;
    const IDX i = sizeof(IDX) == 4 ? (IDX)fast_div((unsigned)r, inv_D) : r / (IDX)D;
    const unsigned l = (unsigned)(r - i * D);
    const uint4 r0 = rec[3 * (size_t)i], r1 = rec[3 * (size_t)i + 1], r2 = rec[3 * (size_t)i + 2];
    const uint64_t leaf0 = u64_of(r0.x, r0.y), nt = u64_of(r0.z, r0.w), lo = u64_of(r1.x, r1.y), leaf = u64_of(r1.z, r1.w);
    const uint64_t c = u64_of(r2.x, r2.y);
    const size_t a = r2.z;
    const bool good = c != 0;
    if (l == 0 && piece < 2) leaves_out[2 * (size_t)i + piece] = good ? leaves[2 * (size_t)(leaf0 + leaf) + piece] : ZERO4;
    // the tree at c leaves has a row l while its level l has more than one node (l < depth(c))
    const bool live = good && ceil_shift(c, l * SHIFT) > 1;
    const uint64_t node = leaf >> (SHIFT * l);  // (l < D <= 64 / SHIFT)
    const unsigned p = (unsigned)(node & (ARITY - 1));
    const uint64_t j = node - p + sib + (sib >= p ? 1u : 0u);  // the group's nodes in order, the path's own node left out
    const uint64_t fc = c >> (SHIFT * l);                      // f_l(c): the nodes of level l that are final at count c
    uint4 v = ZERO4;
    if (live && j < fc) {  // the stored node: level l of the GROWN tree's block (j < f_l(c) <= f_l(n_t))
        const uint64_t first = l == 0 ? leaf0 : lo + level_start(nt, l, SHIFT);
        v = (l == 0 ? leaves : levels)[2 * (size_t)(first + j) + half];
    } else if (live && j == fc && low_bits(c, SHIFT * l) != 0) {  // the partial node P_l(c) (l >= 1: c % 1 == 0)
        v = partial[2 * ((size_t)(l - 1) * m + a) + half];
    }
    siblings[t] = v;
    if (piece == 0) positions[r] = live ? (uint8_t)p : (uint8_t)0;
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api_forest.cpp)
// ---------------------------------------------------------------------------------------------
template <unsigned ARITY>
static hipError_t launch_anchor_pieces(const void* leaves, const void* levels, const void* records, const void* partial, size_t m, size_t k,
                                       unsigned D, void* leaves_out, void* siblings, void* positions, hipStream_t st) {
    const size_t lanes = D ? k * D * 2 * (ARITY - 1) : 2 * k;
    const dim3 grid((unsigned)((lanes + FA_BLOCK - 1) / FA_BLOCK));
    const unsigned long long inv_D = fast_div_reciprocal(D);
    if (lanes + FA_BLOCK <= 0xffffffffull)
        hipLaunchKernelGGL((k_fa_openings<uint32_t, ARITY>), grid, dim3(FA_BLOCK), 0, st, static_cast<const uint4*>(leaves),
                           static_cast<const uint4*>(levels), static_cast<const uint4*>(records), static_cast<const uint4*>(partial), m, k, D,
                           inv_D, static_cast<uint4*>(leaves_out), static_cast<uint4*>(siblings), static_cast<uint8_t*>(positions));
    else
        hipLaunchKernelGGL((k_fa_openings<size_t, ARITY>), grid, dim3(FA_BLOCK), 0, st, static_cast<const uint4*>(leaves),
                           static_cast<const uint4*>(levels), static_cast<const uint4*>(records), static_cast<const uint4*>(partial), m, k, D,
                           inv_D, static_cast<uint4*>(leaves_out), static_cast<uint4*>(siblings), static_cast<uint8_t*>(positions));
    return hipGetLastError();
}

hipError_t launch_forest_anchor_openings(unsigned arity, const int32_t* tab, const TagArg& tag, const void* leaves, const void* levels,
                                         const void* offsets, const uint64_t* ntree, const uint64_t* lo, size_t n_trees,
                                         const void* anchor_tree_ids, const void* anchor_counts, size_t m, const void* anchor_ids,
                                         const void* leaf_ids, size_t k, unsigned stride_depth, void* anchor_roots, void* anchor_depths,
                                         void* leaves_out, void* siblings, void* positions, void* depths, void* n_bad_anchors, void* n_bad,
                                         void* n_hashed, void* work, void* children, hipStream_t st) {
    if (m == 0 && k == 0) return hipSuccess;
    const ForestAnchorWork w = forest_anchor_work(arity, m, k, stride_depth);
    char* base = static_cast<char*>(work);
    uint4* arec = reinterpret_cast<uint4*>(base + w.anchors);
    char* partial = base + w.partial;
    uint4* rec = reinterpret_cast<uint4*>(base + w.records);
    const unsigned la = arity == 4 ? 2u : 1u;
    const dim3 blk(FA_BLOCK);
    if (m) {
        const dim3 per_anchor((unsigned)((m + FA_BLOCK - 1) / FA_BLOCK));
        hipLaunchKernelGGL(k_fa_anchor, per_anchor, blk, 0, st, static_cast<const uint64_t*>(offsets), ntree, lo, n_trees,
                           static_cast<const uint32_t*>(anchor_tree_ids), static_cast<const uint64_t*>(anchor_counts), m, la, arec,
                           static_cast<Scalar32*>(anchor_roots), static_cast<uint8_t*>(anchor_depths), static_cast<unsigned*>(n_bad_anchors),
                           static_cast<unsigned long long*>(n_hashed));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const dim3 per_piece((unsigned)((m * 2 * arity + FA_BLOCK - 1) / FA_BLOCK));
        auto gather = arity == 4 ? k_fa_children<4> : k_fa_children<2>;
        for (unsigned l = 1; l <= stride_depth; ++l) {
            hipLaunchKernelGGL(gather, per_piece, blk, 0, st, static_cast<const uint4*>(leaves), static_cast<const uint4*>(levels), arec,
                               reinterpret_cast<const uint4*>(partial), m, l, static_cast<uint4*>(children));
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            // (the lane-group builds for a batch that cannot fill the chip, the one-lane builds above: launch_merkle4's own rule)
            e = launch_merkle4(tab, tag, children, m * arity, partial + (size_t)(l - 1) * m * 32, m, st, arity);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_fa_roots, per_anchor, blk, 0, st, static_cast<const Scalar32*>(leaves), static_cast<const Scalar32*>(levels), arec,
                           reinterpret_cast<const uint4*>(partial), m, la, static_cast<Scalar32*>(anchor_roots));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fa_record, dim3((unsigned)((k + FA_BLOCK - 1) / FA_BLOCK)), blk, 0, st, arec, m, static_cast<const uint32_t*>(anchor_ids),
                       static_cast<const uint64_t*>(leaf_ids), k, la, rec, static_cast<uint8_t*>(depths), static_cast<unsigned*>(n_bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return arity == 4 ? launch_anchor_pieces<4>(leaves, levels, rec, partial, m, k, stride_depth, leaves_out, siblings, positions, st)
                      : launch_anchor_pieces<2>(leaves, levels, rec, partial, m, k, stride_depth, leaves_out, siblings, positions, st);
}

}  // namespace p252
