// forest_consistency.hip — consistency proofs of the ragged forest: that a tree now of m leaves is the tree it was at n <= m leaves
// with leaves appended and nothing before them changed.  With A = arity, f_l(n) = n / A^l and d_l(n) = f_l(n) % A, the proof of
// (tree, n) is the opening of leaf index n of the tree as it is now (forest_openings.h's layout): its slot on row l is d_l(n), and its
// siblings left of the slot are the nodes [A f_{l+1}(n), f_l(n)) of level l, which are final at count n — row l of the frontier of
// the tree at n leaves (forest_frontier.h).  So ONE opening carries two chains: all of it re-hashes to the new root, its left
// siblings alone to the old root.
//
// Extraction (no hashing):
//   k_fc_record      one lane per proof: k_fo_record's record with the old count as the leaf id, for 1 <= n < n_t; n == n_t (the tree
//                    did not grow) gets an all-zero record, so that the pieces kernel writes zeros, and the depth byte depth(n_t);
//                    a bad proof (tree id >= n_trees, a bad tree, n == 0, n > n_t) gets zeros, depth 0xFF, new count 0, one count.
//                    The pieces are forest_openings.hip's k_fr_openings, through its launcher.
// Verification (no hashing kernel of its own: both chains are walks of k_path_ragged, forest_openings.hip):
//   k_fc_prepare     one lane per (proof, row): the counts and depth checks, and the two walks laid out for k_path_ragged.  The NEW
//                    chain is the proof itself with its slots rewritten as the digits of n — taken from n, never from the proof,
//                    whose position bytes are only compared.  The OLD chain, "the first d_l(n) siblings, then the carried node if
//                    there is one, then zeros", is the walk of an opening whose slot on a level is d_l(n) and whose siblings right
//                    of the slot are zero; it starts from a zero node at the lowest level l0 whose digit of n is non-zero (below
//                    it nothing is hashed) and has depth(n) - l0 rows, so the kernel copies rows l0 .. depth(n) - 1 of the proof,
//                    right siblings zeroed, to rows 0 .. of a second opening.  n == A^depth(n): no row, and that opening's leaf
//                    is sibling 0 of row depth(n), which k_path_ragged reduces as it does a one-leaf tree's root.  Refused and
//                    unchanged proofs get depth 0xFF in both walks: nothing is hashed for them.  The lane of row 0 writes the
//                    status byte and adds the digests to come to one LDS counter per block.
//   k_path_ragged    twice, each sorted by its own depth bytes (P252_RAGGED_SORT=0: identity order): a lane hashes exactly the
//                    digests of its chain, depth(m) and depth(n) - l0
//   k_fc_finish      one lane per proof: both roots against the claimed ones as the 32 bytes they are, the verdict, the roots out
#include <hip/hip_runtime.h>

#include "forest_consistency.h"
#include "forest_node.hpp"
#include "forest_openings.h"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FC_BLOCK = 256;

enum : unsigned { FC_REFUSED = 0, FC_SAME = 1, FC_GROWN = 2, FC_WRONG_SLOTS = 3 };  // a proof's status byte

__device__ __forceinline__ bool eq4(const uint4& a, const uint4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

}  // namespace

// ---- the record of each proof: k_fo_record's two words, {leaf start of the tree, n_t (0: nothing to open), LO[t], leaf id = n} ----
__global__ void __launch_bounds__(FC_BLOCK) k_fc_record(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                        const uint64_t* __restrict__ LO, size_t n_trees,
                                                        const uint32_t* __restrict__ tree_ids, const uint64_t* __restrict__ old_counts,
                                                        size_t k, unsigned la, uint4* __restrict__ rec, uint8_t* __restrict__ depths,
                                                        uint64_t* __restrict__ new_counts, unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= k) return;
    const size_t t = tree_ids[i];
    const uint64_t n = old_counts[i];
    size_t ts;
    const uint64_t nt = forest_tree_leaves(ntree, n_trees, t, &ts);
    const bool good = nt != 0 && n >= 1 && n <= nt;
    const bool open = good && n < nt;  // there is a leaf n to open
    const uint64_t leaf0 = open ? offsets[ts] : 0ull, lo = open ? LO[ts] : 0ull, nn = open ? nt : 0ull, lf = open ? n : 0ull;
    unsigned d = 0;  // p252_merkle{4,2}_depth(n_t)
#pragma unroll 1
    for (uint64_t c = good ? nt : 0ull; c > 1; c = ceil_shift(c, la)) ++d;
    rec[2 * i] = make_uint4((unsigned)leaf0, (unsigned)(leaf0 >> 32), (unsigned)nn, (unsigned)(nn >> 32));
    rec[2 * i + 1] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)lf, (unsigned)(lf >> 32));
    depths[i] = good ? (uint8_t)d : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
    new_counts[i] = good ? nt : 0ull;
    if (!good && n_bad) atomicAdd(n_bad, 1u);
}

// ---- the two walks of each proof, laid out for k_path_ragged.  Lane (i, j) = proof i, row j of the stride (one lane per proof when
// the stride is 0).  Every lane works out its proof's counts; the lane of row 0 also writes what the proof has once. ----
template <unsigned ARITY>
__global__ void __launch_bounds__(FC_BLOCK) k_fc_prepare(const uint64_t* __restrict__ old_counts, const uint64_t* __restrict__ new_counts,
                                                         const uint4* __restrict__ siblings, const uint8_t* __restrict__ positions,
                                                         const uint8_t* __restrict__ depths, unsigned stride,
                                                         const uint32_t* __restrict__ tree_ids, size_t n_claims, size_t k,
                                                         uint4* __restrict__ o_leaves, uint4* __restrict__ o_sib, uint8_t* __restrict__ o_pos,
                                                         uint8_t* __restrict__ o_dep, uint8_t* __restrict__ n_pos, uint8_t* __restrict__ n_dep,
                                                         uint8_t* __restrict__ status, unsigned long long* __restrict__ n_hashed) {
    constexpr unsigned SHIFT = ARITY == 4 ? 2 : 1, PER = ARITY - 1;
    __shared__ unsigned block_hashed;
    if (threadIdx.x == 0) block_hashed = 0;
    __syncthreads();
    const unsigned rows = stride ? stride : 1u;
    const size_t t = (size_t)blockIdx.x * FC_BLOCK + threadIdx.x;
    const size_t i = t / rows;
    const unsigned j = (unsigned)(t - i * rows);
    unsigned hashed = 0;
    if (i < k) {
        const size_t c = tree_ids ? (size_t)tree_ids[i] : i;
        uint64_t n = 0, m = 0;
        if (c < n_claims) {
            n = old_counts[c];
            m = new_counts[c];
        }
        unsigned dm = 0, dn = 0;  // p252_merkle{4,2}_depth of m and of n
#pragma unroll 1
        for (uint64_t w = m; w > 1; w = ceil_shift(w, SHIFT)) ++dm;
#pragma unroll 1
        for (uint64_t w = n; w > 1; w = ceil_shift(w, SHIFT)) ++dn;
        const bool valid = n != 0 && n <= m && depths[i] == dm && dm <= stride;  // (an unknown claim has n == 0)
        const bool grown = valid && n < m;  // then dn <= dm <= stride, and dn < dm whenever n == A^dn
        unsigned l0 = 0;  // the lowest level whose digit of n is non-zero; dn when n == A^dn: the old chain hashes nothing
#pragma unroll 1
        while (l0 < dn && ((n >> (SHIFT * l0)) & (ARITY - 1)) == 0) ++l0;
        const unsigned od = dn - l0;  // digests of the old chain = rows of its walk
        if (stride) {
            const unsigned l = l0 + j;  // row j of the old walk is row l of the proof, its right siblings zeroed
            const bool live = grown && l < dn;
            const unsigned d = live ? (unsigned)(n >> (SHIFT * l)) & (ARITY - 1) : 0u;
            const size_t dst = (i * stride + j) * PER * 2, src = (i * stride + (live ? l : 0u)) * PER * 2;
#pragma unroll
            for (unsigned q = 0; q < PER * 2; ++q) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (live && (q >> 1) < d) v = siblings[src + q];
                o_sib[dst + q] = v;
            }
            o_pos[i * stride + j] = (uint8_t)d;
            n_pos[i * stride + j] = (grown && j < dm) ? (uint8_t)((n >> (SHIFT * j)) & (ARITY - 1)) : (uint8_t)0;
        }
        if (j == 0) {
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;  // the old walk starts from nothing; n == A^dn: from the final node itself
            if (grown && od == 0) {
                a = siblings[(i * stride + dn) * PER * 2];
                b = siblings[(i * stride + dn) * PER * 2 + 1];
            }
            o_leaves[2 * i] = a;
            o_leaves[2 * i + 1] = b;
            o_dep[i] = grown ? (uint8_t)od : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
            n_dep[i] = grown ? (uint8_t)dm : (uint8_t)FOREST_OPENINGS_BAD_DEPTH;
            unsigned pos_bad = 0;
            if (grown) {
#pragma unroll 1
                for (unsigned l = 0; l < dm; ++l) pos_bad |= (unsigned)positions[i * stride + l] ^ ((unsigned)(n >> (SHIFT * l)) & (ARITY - 1));
                hashed = dm + od;
            }
            status[i] = !valid ? FC_REFUSED : !grown ? FC_SAME : pos_bad ? FC_WRONG_SLOTS : FC_GROWN;
        }
    }
    if (!n_hashed) return;  // (uniform)
    if (hashed) atomicAdd(&block_hashed, hashed);  // one global atomic per block
    __syncthreads();
    if (threadIdx.x == 0 && block_hashed) atomicAdd(n_hashed, (unsigned long long)block_hashed);
}

// ---- the verdicts: both recomputed roots against the claimed ones, as the 32 bytes they are ----
__global__ void __launch_bounds__(FC_BLOCK) k_fc_finish(const uint8_t* __restrict__ status, const uint32_t* __restrict__ tree_ids,
                                                        const uint4* __restrict__ old_roots, const uint4* __restrict__ new_roots,
                                                        const uint4* __restrict__ got_old, const uint4* __restrict__ got_new,
                                                        uint8_t* __restrict__ ok, uint4* __restrict__ old_out, uint4* __restrict__ new_out, size_t k) {
    const size_t i = (size_t)blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= k) return;
    const unsigned st = status[i];
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    uint4 a0 = zero, a1 = zero, b0 = zero, b1 = zero;  // what goes out: zero for a refused proof
    bool same = false;
    if (st != FC_REFUSED) {
        const size_t c = tree_ids ? (size_t)tree_ids[i] : i;  // (k_fc_prepare found it inside the claims)
        const uint4 oa = old_roots[2 * c], ob = old_roots[2 * c + 1], na = new_roots[2 * c], nb = new_roots[2 * c + 1];
        if (st == FC_SAME) {  // the tree did not grow: the claimed roots themselves
            a0 = oa, a1 = ob, b0 = na, b1 = nb;
            same = eq4(oa, na) && eq4(ob, nb);
        } else {
            a0 = got_old[2 * i], a1 = got_old[2 * i + 1], b0 = got_new[2 * i], b1 = got_new[2 * i + 1];
            same = st == FC_GROWN && eq4(a0, oa) && eq4(a1, ob) && eq4(b0, na) && eq4(b1, nb);
        }
    }
    ok[i] = same ? (uint8_t)1 : (uint8_t)0;
    if (old_out) old_out[2 * i] = a0, old_out[2 * i + 1] = a1;
    if (new_out) new_out[2 * i] = b0, new_out[2 * i + 1] = b1;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
hipError_t launch_forest_consistency_extract(unsigned arity, const void* leaves, const void* levels, const void* offsets,
                                             const uint64_t* ntree, const uint64_t* lo, size_t n_trees, const void* tree_ids,
                                             const void* old_counts, size_t k, unsigned stride_depth, void* records, void* new_counts_out,
                                             void* leaves_out, void* siblings, void* positions, void* depths, void* n_bad, hipStream_t st) {
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fc_record, dim3((unsigned)((k + FC_BLOCK - 1) / FC_BLOCK)), dim3(FC_BLOCK), 0, st,
                       static_cast<const uint64_t*>(offsets), ntree, lo, n_trees, static_cast<const uint32_t*>(tree_ids),
                       static_cast<const uint64_t*>(old_counts), k, arity == 4 ? 2u : 1u, static_cast<uint4*>(records),
                       static_cast<uint8_t*>(depths), static_cast<uint64_t*>(new_counts_out), static_cast<unsigned*>(n_bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_forest_opening_pieces(arity, leaves, levels, records, k, stride_depth, leaves_out, siblings, positions, st);
}

hipError_t launch_forest_consistency_verify(unsigned arity, const int32_t* tab, const TagArg& tag, const void* old_counts,
                                            const void* old_roots, const void* new_counts, const void* new_roots, const void* leaves,
                                            const void* siblings, const void* positions, const void* depths, unsigned stride_depth, size_t k,
                                            const void* tree_ids, size_t n_claims, void* ok, void* old_roots_out, void* new_roots_out,
                                            void* n_hashed, void* work, void* hist, bool sort, hipStream_t st) {
    if (k == 0) return hipSuccess;
    const ForestConsistencyWork w = forest_consistency_work(arity, k, stride_depth);
    char* base = static_cast<char*>(work);
    uint4* o_leaves = reinterpret_cast<uint4*>(base + w.o_leaves);
    uint4* o_sib = reinterpret_cast<uint4*>(base + w.o_sib);
    uint4* got_old = reinterpret_cast<uint4*>(base + w.got_old);
    uint4* got_new = reinterpret_cast<uint4*>(base + w.got_new);
    uint8_t *o_pos = reinterpret_cast<uint8_t*>(base + w.o_pos), *n_pos = reinterpret_cast<uint8_t*>(base + w.n_pos);
    uint8_t *o_dep = reinterpret_cast<uint8_t*>(base + w.o_dep), *n_dep = reinterpret_cast<uint8_t*>(base + w.n_dep);
    uint8_t* status = reinterpret_cast<uint8_t*>(base + w.status);
    void* order = sort ? base + w.order : nullptr;
    const size_t claims = tree_ids ? n_claims : k;
    const size_t lanes = k * (stride_depth ? stride_depth : 1u);
    const dim3 grid((unsigned)((lanes + FC_BLOCK - 1) / FC_BLOCK));
    auto prep = arity == 4 ? k_fc_prepare<4> : k_fc_prepare<2>;
    hipLaunchKernelGGL(prep, grid, dim3(FC_BLOCK), 0, st, static_cast<const uint64_t*>(old_counts), static_cast<const uint64_t*>(new_counts),
                       static_cast<const uint4*>(siblings), static_cast<const uint8_t*>(positions), static_cast<const uint8_t*>(depths), stride_depth,
                       static_cast<const uint32_t*>(tree_ids), claims, k, o_leaves, o_sib, o_pos, o_dep, n_pos, n_dep, status,
                       static_cast<unsigned long long*>(n_hashed));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the new chain: the proof itself with its slots taken from n; the old chain: its left siblings alone.  Each sorted by its own depths.
    e = launch_path_ragged(arity, tab, tag, leaves, siblings, n_pos, n_dep, stride_depth, got_new, k, nullptr, order, sort ? hist : nullptr, st);
    if (e != hipSuccess) return e;
    e = launch_path_ragged(arity, tab, tag, o_leaves, o_sib, o_pos, o_dep, stride_depth, got_old, k, nullptr, order, sort ? hist : nullptr, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fc_finish, dim3((unsigned)((k + FC_BLOCK - 1) / FC_BLOCK)), dim3(FC_BLOCK), 0, st, status,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint4*>(old_roots), static_cast<const uint4*>(new_roots), got_old,
                       got_new, static_cast<uint8_t*>(ok), static_cast<uint4*>(old_roots_out), static_cast<uint4*>(new_roots_out), k);
    return hipGetLastError();
}

}  // namespace p252
