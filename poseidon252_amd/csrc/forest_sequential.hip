// forest_sequential.hip — k leaf updates of a built ragged forest (forest_ragged.hip, tree-major levels) applied IN ORDER in one call,
// for both arities: update i sees the forest as updates 0 .. i - 1 left it, and gets its witness — the leaf it replaces, the opening of
// that leaf in the state just before it, the tree's root before and after.  Every intermediate root is a different value, so the call
// costs one digest per update and level whatever the method; the method makes them parallel level by level.
//
// The list.  The updates are kept as a list sorted by (tree, node, time): time = the update's index, node = its leaf, then that leaf's
// ancestor level by level.  A RUN is the elements of one (tree, node), ascending in time; the element of update i holds the value of its
// node just after update i.  The caller's d_order is the list of level 0 (the stable sort by pair); the library checks it and sorts
// nothing.  With A = arity, on level l an element (t, c, i) needs, for every other child slot n of its parent c / A:
//   the value of n as of time i = the value of the last element of run (t, n) with time < i — one binary search for the first key
//   >= (t, n, i) — or, when the run has none, the STORED node, or zero at and past the level's width.
// Those A - 1 values are row l of update i's opening; with the element's own value they are the A children whose digest is the value of
// the parent just after update i.  The parents' list must again be sorted by (tree, parent, time): an element's new place is the start
// of its parent's group (the runs of the parent's A children are neighbours in the list) plus, over those runs, the number of elements
// with time < i — binary searches again, no sort: the MERGE RANK.
//   k_sq_check     one lane per place of d_order: the order is valid iff every entry is < k and (tree, leaf, index) ascends strictly
//                  from place to place, which makes it a permutation; an invalid order sets ctr[SQ_BAD], and every later kernel
//                  leaves at once (the forest and the outputs stay untouched, but for what k_sq_finish says).  Writes the key and the
//                  value (the new leaf) of the level-0 list, nothing of the caller's.
//   k_sq_gather    level l, one lane per (element, child slot): the child's value as of the element's time into children[k][A], the
//                  sibling row and position byte of the witness, and per slot the two words of the merge rank (the first key >= (t, n, i)
//                  and the elements of run (t, n) before it).  Level 0 also writes the old leaf, the depth byte, both roots of a
//                  one-leaf tree's update, a bad update's zero rows, and counts.
//   (launch_merkle4 over those k nodes: the parents' values, in the list's order.  No hashing kernel of this unit's own — every
//    hashing kernel has its row in the edge-value matrix of the tests; the launcher also picks the lane-group or the one-lane build.)
//   k_sq_rank      level l, one lane per element: WRITE-BACK — the last element of a run stores its value to the stored node (leaf,
//                  level node, and d_roots for a root) —, then the merge rank and the scatter of key and parent's value into the list of
//                  level l + 1; an element whose parent is its tree's root deposits roots_after and roots_before (the parent's value
//                  of the latest earlier element of the whole group, or the stored root).
//   k_sq_finish    one lane per element: the write-back of the last level's list; after an invalid order every depth byte 0xFF and
//                  k bad updates.
// THE HAZARD: the stored nodes of level l are what k_sq_gather of level l reads when a run has no earlier element, so the write-back of
// level l runs in k_sq_rank of level l: a later launch.  (k_sq_rank reads stored nodes of level l + 1 only — the stored root.)
// Elements of bad updates (node 0xFFFFFFFF: behind every good element of their tree, never searched for) and of trees that ended below
// level l keep their place and their key; their children are zeros, digested and dropped, as the anchors of forest_anchor.hip.
#include <hip/hip_runtime.h>

#include "forest_node.hpp"
#include "forest_openings.h"
#include "forest_sequential.h"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned SQ_BLOCK = 256;
constexpr unsigned SQ_BAD = 0;               // ctr[SQ_BAD]: the order is invalid
constexpr size_t SQ_COUNT_BYTES = 256;       // the counters' room at the head of the work area
constexpr uint32_t SQ_NO_NODE = 0xffffffffu;  // the node of a bad update's element (a good node is < max_leaves < 2^32)
constexpr unsigned SQ_BAD_DEPTH = FOREST_OPENINGS_BAD_DEPTH;

#define ZERO4 make_uint4(0u, 0u, 0u, 0u)

// a key {tree, node, time, depth of the tree (SQ_BAD_DEPTH: a bad update)} against (t, n, i)
__device__ __forceinline__ bool key_below(const uint4 key, uint32_t t, uint32_t n, uint32_t i) {
    return key.x != t ? key.x < t : key.y != n ? key.y < n : key.z < i;
}
// the first place in [0, hi) whose key is >= (t, n, i); hi where there is none
__device__ __forceinline__ uint32_t first_not_below(const uint4* __restrict__ keys, uint32_t hi, uint32_t t, uint32_t n, uint32_t i) {
    uint32_t lo = 0;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key_below(keys[mid], t, n, i))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned depth_of(uint64_t n, unsigned la) {
    unsigned d = 0;
#pragma unroll 1
    for (uint64_t w = n; w > 1; w = ceil_shift(w, la)) ++d;
    return d;
}

// the forest as the call was given it, behind its index
struct SqForest {
    uint4* leaves;
    uint4* levels;
    uint4* roots;  // (may be null)
    const uint64_t* offsets;
    const uint64_t* ntree;
    const uint64_t* lo;
};
// the stored node c of level l of tree t of n leaves (l == 0: the leaf)
__device__ __forceinline__ uint4* stored_node(const SqForest& F, uint32_t t, uint64_t n, unsigned l, uint32_t c, unsigned la) {
    return l == 0 ? F.leaves + 2 * (size_t)(F.offsets[t] + c) : F.levels + 2 * (size_t)(F.lo[t] + level_start(n, l, la) + c);
}

}  // namespace

// ---- the order and the pairs; the list of level 0 ----
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_check(const uint64_t* __restrict__ ntree, size_t n_trees, const uint32_t* __restrict__ tree_ids,
                                                       const uint64_t* __restrict__ leaf_ids, const uint4* __restrict__ new_leaves,
                                                       const uint32_t* __restrict__ order, uint32_t k, unsigned la, unsigned* __restrict__ ctr,
                                                       uint4* __restrict__ keys, uint4* __restrict__ vals) {
    const size_t p = (size_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (p >= k) return;
    const uint32_t i = order[p];
    bool valid = i < k;
    uint32_t t = 0;
    uint64_t leaf = 0;
    if (valid) {
        t = tree_ids[i];
        leaf = leaf_ids[i];
        if (p > 0) {  // (tree, leaf, index) ascends strictly from the place before
            const uint32_t j = order[p - 1];
            if (j >= k) {
                valid = false;
            } else {
                const uint32_t tj = tree_ids[j];
                const uint64_t lj = leaf_ids[j];
                valid = tj != t ? tj < t : lj != leaf ? lj < leaf : j < i;
            }
        }
    }
    if (!valid) {
        ctr[SQ_BAD] = 1;  // (every later kernel leaves at once: what this lane would write is never read)
        return;
    }
    size_t ts;
    const uint64_t nt = forest_tree_leaves(ntree, n_trees, t, &ts);
    const bool good = nt != 0 && leaf < nt;
    keys[p] = make_uint4(t, good ? (uint32_t)leaf : SQ_NO_NODE, i, good ? depth_of(nt, la) : SQ_BAD_DEPTH);
    vals[2 * p] = new_leaves[2 * (size_t)i];
    vals[2 * p + 1] = new_leaves[2 * (size_t)i + 1];
}

// ---- level l: the children of every element's parent as of the element's time, the witness row, the words of the merge rank ----
template <unsigned ARITY>
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_gather(SqForest F, const unsigned* __restrict__ ctr, const uint4* __restrict__ keys,
                                                        const uint4* __restrict__ vals, uint32_t k, unsigned l, unsigned D,
                                                        uint4* __restrict__ children, uint2* __restrict__ ranks, uint4* __restrict__ old_leaves,
                                                        uint4* __restrict__ siblings, uint8_t* __restrict__ positions,
                                                        uint8_t* __restrict__ depths, uint4* __restrict__ roots_before,
                                                        uint4* __restrict__ roots_after, unsigned* __restrict__ n_bad,
                                                        unsigned long long* __restrict__ n_hashed) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    __shared__ unsigned block_hashed;
    if (ctr[SQ_BAD]) return;  // (the whole grid)
    if (threadIdx.x == 0) block_hashed = 0;
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * SQ_BLOCK + threadIdx.x;  // = the index of the scalar of `children` this lane stores
    const uint32_t p = (uint32_t)(g / ARITY);
    const unsigned j = (unsigned)(g % ARITY);
    unsigned hashed = 0;
    if (g < (size_t)k * ARITY) {
        const uint4 key = keys[p];
        const uint32_t t = key.x, c = key.y, i = key.z;
        const unsigned d = key.w;
        const bool good = d != SQ_BAD_DEPTH, live = good && l < d;
        const uint64_t nt = good ? F.ntree[t] : 0;
        const unsigned own = live ? c & (ARITY - 1) : 0u;
        uint4 v0 = ZERO4, v1 = ZERO4;
        if (live && j != own) {
            const uint32_t n = c - own + j;
            uint2 rank = make_uint2(0u, 0u);
            if (n < ceil_shift(nt, l * LA)) {  // (at and past the level's width: zero, and the run is empty)
                const uint32_t e = first_not_below(keys, k, t, n, i), s = first_not_below(keys, e, t, n, 0u);
                rank = make_uint2(e, e - s);
                const uint4* src = e > s ? vals + 2 * (size_t)(e - 1) : stored_node(F, t, nt, l, n, LA);
                v0 = src[0];
                v1 = src[1];
            }
            ranks[g] = rank;
        } else if (j == own && (live || l == 0)) {  // the element's own slot (slot 0 of an element that has no parent)
            const uint32_t s = good ? first_not_below(keys, p, t, c, 0u) : p;
            if (live) {
                ranks[g] = make_uint2(p, p - s);
                v0 = vals[2 * (size_t)p];
                v1 = vals[2 * (size_t)p + 1];
            }
            if (l == 0) {  // the witness's head, once per update
                uint4 o0 = ZERO4, o1 = ZERO4;
                if (good) {  // the leaf as stored just before update i: the element before in its run, or the stored leaf
                    const uint4* src = p > s ? vals + 2 * (size_t)(p - 1) : stored_node(F, t, nt, 0, c, LA);
                    o0 = src[0];
                    o1 = src[1];
                    hashed = d;
                } else if (n_bad) {
                    atomicAdd(n_bad, 1u);
                }
                if (old_leaves) {
                    old_leaves[2 * (size_t)i] = o0;
                    old_leaves[2 * (size_t)i + 1] = o1;
                }
                depths[i] = (uint8_t)d;
                if (!good || d == 0) {  // a bad update's roots: zero; a one-leaf tree's: the leaf mod p, before and after
                    uint4 a0 = ZERO4, a1 = ZERO4;
                    if (good) {
                        a0 = vals[2 * (size_t)p];
                        a1 = vals[2 * (size_t)p + 1];
                        words_mod_p(o0, o1);
                        words_mod_p(a0, a1);
                    }
                    if (roots_before) {
                        roots_before[2 * (size_t)i] = o0;
                        roots_before[2 * (size_t)i + 1] = o1;
                    }
                    roots_after[2 * (size_t)i] = a0;
                    roots_after[2 * (size_t)i + 1] = a1;
                }
            }
        }
        if (l < D) {
            children[2 * g] = v0;
            children[2 * g + 1] = v1;
            const size_t row = (size_t)i * D + l;
            if (j == own) {
                positions[row] = (uint8_t)own;
            } else {
                const size_t at = row * (ARITY - 1) + (j < own ? j : j - 1);
                siblings[2 * at] = v0;
                siblings[2 * at + 1] = v1;
            }
        }
    }
    if (l != 0 || !n_hashed) return;  // (uniform)
    if (hashed) atomicAdd(&block_hashed, hashed);  // one global atomic per block
    __syncthreads();
    if (threadIdx.x == 0 && block_hashed) atomicAdd(n_hashed, (unsigned long long)block_hashed);
}

// the write-back of level l: the last element of a run holds the node's final value
__device__ __forceinline__ void write_back(const SqForest& F, const uint4* __restrict__ keys, const uint4* __restrict__ vals, uint32_t k,
                                           uint32_t p, const uint4 key, unsigned l, unsigned la) {
    if (p + 1 < k) {
        const uint4 next = keys[p + 1];
        if (next.x == key.x && next.y == key.y) return;
    }
    const uint64_t nt = F.ntree[key.x];
    uint4 v0 = vals[2 * (size_t)p], v1 = vals[2 * (size_t)p + 1];
    uint4* dst = stored_node(F, key.x, nt, l, key.y, la);
    dst[0] = v0;
    dst[1] = v1;
    if (l == key.w && F.roots) {  // the tree's root (a one-leaf tree's: its leaf mod p)
        if (l == 0) words_mod_p(v0, v1);
        F.roots[2 * (size_t)key.x] = v0;
        F.roots[2 * (size_t)key.x + 1] = v1;
    }
}

// ---- level l -> l + 1: the write-back of level l, the merge rank, the list of level l + 1, the roots of the trees that end there ----
template <unsigned ARITY>
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_rank(SqForest F, const unsigned* __restrict__ ctr, const uint4* __restrict__ keys,
                                                      const uint4* __restrict__ vals, const uint4* __restrict__ parents,
                                                      const uint2* __restrict__ ranks, uint32_t k, unsigned l, uint4* __restrict__ keys_up,
                                                      uint4* __restrict__ vals_up, uint4* __restrict__ roots_before,
                                                      uint4* __restrict__ roots_after) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    if (ctr[SQ_BAD]) return;  // (the whole grid)
    const size_t at_p = (size_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (at_p >= k) return;
    const uint32_t p = (uint32_t)at_p;
    const uint4 key = keys[p];
    const unsigned d = key.w;
    if (d == SQ_BAD_DEPTH || l > d) {  // a bad update, or a tree that ended below: the element keeps its place and its key
        keys_up[p] = key;
        return;
    }
    write_back(F, keys, vals, k, p, key, l, LA);
    if (l == d) {
        keys_up[p] = key;
        return;
    }
    // the parent's group starts where the run of its first child starts; then the elements of the group's runs that are earlier
    uint2 r[ARITY];
#pragma unroll
    for (unsigned j = 0; j < ARITY; ++j) r[j] = ranks[(size_t)p * ARITY + j];
    uint32_t q = r[0].x - r[0].y;
#pragma unroll
    for (unsigned j = 0; j < ARITY; ++j) q += r[j].y;
    const uint4 up0 = parents[2 * (size_t)p], up1 = parents[2 * (size_t)p + 1];
    keys_up[q] = make_uint4(key.x, key.y >> LA, key.z, d);
    vals_up[2 * (size_t)q] = up0;
    vals_up[2 * (size_t)q + 1] = up1;
    if (d != l + 1) return;
    // the parent is the root, and the group the whole tree: the root before update i is the parent's value of the latest earlier element
    roots_after[2 * (size_t)key.z] = up0;
    roots_after[2 * (size_t)key.z + 1] = up1;
    if (!roots_before) return;
    bool found = false;
    uint32_t latest = 0, at = 0;
#pragma unroll
    for (unsigned j = 0; j < ARITY; ++j) {
        if (r[j].y == 0) continue;
        const uint32_t time = keys[r[j].x - 1].z;
        if (!found || time > latest) {
            found = true;
            latest = time;
            at = r[j].x - 1;
        }
    }
    const uint4* src = found ? parents + 2 * (size_t)at : stored_node(F, key.x, F.ntree[key.x], d, 0u, LA);
    roots_before[2 * (size_t)key.z] = src[0];
    roots_before[2 * (size_t)key.z + 1] = src[1];
}

// ---- the write-back of the last level; the verdict on an invalid order ----
__global__ void __launch_bounds__(SQ_BLOCK) k_sq_finish(SqForest F, const unsigned* __restrict__ ctr, const uint4* __restrict__ keys,
                                                        const uint4* __restrict__ vals, uint32_t k, unsigned D, unsigned la,
                                                        uint8_t* __restrict__ depths, unsigned* __restrict__ n_bad) {
    const size_t at_p = (size_t)blockIdx.x * SQ_BLOCK + threadIdx.x;
    if (at_p >= k) return;
    const uint32_t p = (uint32_t)at_p;
    if (ctr[SQ_BAD]) {  // the batch is one object: nothing was applied
        depths[p] = (uint8_t)SQ_BAD_DEPTH;
        if (p == 0 && n_bad) atomicAdd(n_bad, k);
        return;
    }
    const uint4 key = keys[p];
    if (key.w == D) write_back(F, keys, vals, k, p, key, D, la);
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api_forest.cpp)
// ---------------------------------------------------------------------------------------------
hipError_t launch_forest_update_sequential(unsigned arity, const int32_t* tab, const TagArg& tag, void* leaves, const void* offsets,
                                           const uint64_t* ntree, const uint64_t* lo, size_t n_trees, void* levels, const void* tree_ids,
                                           const void* leaf_ids, const void* new_leaves, const void* order, size_t k, unsigned stride_depth,
                                           void* old_leaves, void* siblings, void* positions, void* depths, void* roots_before,
                                           void* roots_after, void* roots, void* n_bad, void* n_hashed, void* work, void* children,
                                           hipStream_t st) {
    if (k == 0) return hipSuccess;
    const ForestSequentialWork w = forest_sequential_work(arity, k);
    char* base = static_cast<char*>(work);
    unsigned* ctr = reinterpret_cast<unsigned*>(base + w.ctr);
    uint4* keys[2] = {reinterpret_cast<uint4*>(base + w.keys[0]), reinterpret_cast<uint4*>(base + w.keys[1])};
    uint4* vals[2] = {reinterpret_cast<uint4*>(base + w.vals[0]), reinterpret_cast<uint4*>(base + w.vals[1])};
    uint4* parents = reinterpret_cast<uint4*>(base + w.parents);
    uint2* ranks = reinterpret_cast<uint2*>(base + w.ranks);
    SqForest F;
    F.leaves = static_cast<uint4*>(leaves);
    F.levels = static_cast<uint4*>(levels);
    F.roots = static_cast<uint4*>(roots);
    F.offsets = static_cast<const uint64_t*>(offsets);
    F.ntree = ntree;
    F.lo = lo;
    const unsigned la = arity == 4 ? 2u : 1u, D = stride_depth;
    const uint32_t k32 = (uint32_t)k;
    const dim3 blk(SQ_BLOCK), per_element((unsigned)((k + SQ_BLOCK - 1) / SQ_BLOCK)), per_slot((unsigned)((k * arity + SQ_BLOCK - 1) / SQ_BLOCK));
    hipError_t e = hipMemsetAsync(ctr, 0, SQ_COUNT_BYTES, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sq_check, per_element, blk, 0, st, ntree, n_trees, static_cast<const uint32_t*>(tree_ids),
                       static_cast<const uint64_t*>(leaf_ids), static_cast<const uint4*>(new_leaves), static_cast<const uint32_t*>(order), k32, la,
                       ctr, keys[0], vals[0]);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    auto gather = arity == 4 ? k_sq_gather<4> : k_sq_gather<2>;
    auto rank = arity == 4 ? k_sq_rank<4> : k_sq_rank<2>;
    for (unsigned l = 0; l < (D ? D : 1u); ++l) {  // (D == 0: the heads of the witnesses alone)
        const unsigned a = l & 1, b = a ^ 1;
        hipLaunchKernelGGL(gather, per_slot, blk, 0, st, F, ctr, keys[a], vals[a], k32, l, D, static_cast<uint4*>(children), ranks,
                           static_cast<uint4*>(old_leaves), static_cast<uint4*>(siblings), static_cast<uint8_t*>(positions),
                           static_cast<uint8_t*>(depths), static_cast<uint4*>(roots_before), static_cast<uint4*>(roots_after),
                           static_cast<unsigned*>(n_bad), static_cast<unsigned long long*>(n_hashed));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (D == 0) break;
        // (the lane-group builds for a batch that cannot fill the chip, the one-lane builds above: launch_merkle4's own rule)
        e = launch_merkle4(tab, tag, children, k * arity, parents, k, st, arity);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rank, per_element, blk, 0, st, F, ctr, keys[a], vals[a], parents, ranks, k32, l, keys[b], vals[b],
                           static_cast<uint4*>(roots_before), static_cast<uint4*>(roots_after));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sq_finish, per_element, blk, 0, st, F, ctr, keys[D & 1], vals[D & 1], k32, D, la, static_cast<uint8_t*>(depths),
                       static_cast<unsigned*>(n_bad));
    return hipGetLastError();
}

}  // namespace p252
