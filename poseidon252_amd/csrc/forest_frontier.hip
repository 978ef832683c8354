// forest_frontier.hip — leaves appended to a forest of Merkle trees of DIFFERENT sizes that is kept only as its frontiers, for both
// arities (p252_merkle{4,2}_forest_frontier_append_device_into), and that state taken out of a built ragged forest
// (p252_merkle{4,2}_forest_frontier_extract_device_into).  With A = arity, f_l(n) = floor(n / A^l), c_l(n) = ceil(n / A^l) and d_l(n) =
// f_l(n) mod A, node j of level l of a tree of n leaves is final iff j < f_l(n), and the final nodes a later append still reads are,
// per level, the d_l(n) nodes [A f_{l+1}(n), f_l(n)) to the right of the last complete group: row l of the tree's frontier (rows
// 0 .. D(max_leaves) of A - 1 scalars, the slots past d_l(n) zero).  An append of m > 0 leaves (n' = n + m) computes, level by level,
// V_{l+1} = the nodes [f_{l+1}(n), c_{l+1}(n')) in index order from V_l (V_0 = the new leaves): the first d_l(n) children of node
// f_{l+1}(n) are the frontier's row l, every other child is in V_l, children at or past c_l(n') are zero; level D(n') has one node,
// the root.  That is sum over l >= 1 of c_l(n') - f_l(n) digests per tree that grows: the stored append's own count (forest_append.hip).
//   k_ff_sizes        per tree: n_t and the append m_t, or "refused" (decreasing add offsets, a range past n_add, n_t > max_leaves,
//                     n_t + m_t > max_leaves)
//   (forest_append_scan_sum_rule: the stored append's own scan over the trees — an append that takes the running sum of the
//                     appends before it past n_add is refused as well, which keeps every level's list within the host's bound)
//   k_ff_refused      per tree: one count in *n_bad for an append refused by either step
//   (forest_append_scan_dirty_lists: the stored append's scans of every level's node count — row l = where tree t's run of V_l
//                     starts — and its expansion, one lane per NODE of a level's list: (tree, node index))
//   k_ff_records      every level at once (gridDim.y), one lane per node: that record rewritten in multiproof.hip's format (the parent
//                     index and the width of the level below are relative to the tree's first computed node, so 32 bits hold them) —
//                     the masked child slots are a run of V_{l-1}, the others the frontier's row l - 1, handed to the digests as
//                     their `proof`
//   (launch_multiproof_digest_list per level: multiproof.hip's k_mp_digest / k_mp_digest_coop.  No kernel here hashes, scans or
//                     searches: the scans and the search are forest_append.hip's, which are blockops.hpp's.)
//   k_ff_finish       after the last digest launch, one lane per (tree, row): the new row l — where f_{l+1} did not move the old
//                     entries stay and V_l[0 .. f_l(n') - f_l(n)) follow them, else the row is V_l[A f_{l+1}(n') - f_l(n) ..) — from
//                     V_l alone, so the state is updated in place; and per tree the root (the top node, or the lone leaf reduced, as
//                     forest_ragged.hip writes a one-leaf tree's), the new count, and the digest count
//   k_ff_extract      one lane per (tree, row) of a built forest: the row out of the tree's leaves or its tree-major block
#include <hip/hip_runtime.h>

#include "forest_append.h"
#include "forest_frontier.h"
#include "forest_node.hpp"
#include "forest_witness.h"
#include "multiproof.h"

namespace p252 {

namespace {

constexpr unsigned FF_BLOCK = FOREST_FRONTIER_BLOCK;
constexpr uint64_t FF_REFUSED = FOREST_APPEND_REFUSED;
constexpr unsigned FF_MASK_SHIFT = 28;  // a record's last word: proof offset bits 32 .. 59, slot mask above (multiproof.hip's)

struct FfTrees {
    uint64_t* nold;  // n_t
    uint64_t* madd;  // m_t (FF_REFUSED between k_ff_sizes and the sum rule)
    uint64_t* pre;   // what k_ff_sizes decided: m_t + 1, or FF_REFUSED — never zero
    size_t n_trees;
    uint64_t n_add;
    unsigned la, depth;
};

__device__ __forceinline__ uint64_t floor_shift(uint64_t n, unsigned k) { return k >= 64 ? 0ull : n >> k; }

__device__ __forceinline__ void copy_scalar(uint4* __restrict__ dst, const uint4* __restrict__ src) {
    dst[0] = src[0];
    dst[1] = src[1];
}

}  // namespace

// ---- per tree: the leaf count and the append ----
__global__ void __launch_bounds__(FF_BLOCK) k_ff_sizes(const uint64_t* __restrict__ counts, const uint64_t* __restrict__ add_offsets,
                                                       uint64_t max_leaves, FfTrees T) {
    const size_t t = (size_t)blockIdx.x * FF_BLOCK + threadIdx.x;
    if (t >= T.n_trees) return;
    const uint64_t n = counts[t];
    const uint64_t lo = add_offsets[t], hi = add_offsets[t + 1];
    const uint64_t m = hi - lo;
    // (n > max_leaves: a corrupt state — refused whatever it is given, so that no later kernel looks past the tree's rows)
    const bool ok = hi >= lo && hi <= T.n_add && n <= max_leaves && m <= max_leaves - n;
    T.nold[t] = n;
    T.madd[t] = ok ? m : FF_REFUSED;
    T.pre[t] = ok ? m + 1 : FF_REFUSED;  // (m <= n_add < 2^32)
}

// ---- the refusals, once the sum rule has settled m_t ----
__global__ void __launch_bounds__(FF_BLOCK) k_ff_refused(FfTrees T, unsigned* __restrict__ n_bad) {
    const size_t t = (size_t)blockIdx.x * FF_BLOCK + threadIdx.x;
    if (t >= T.n_trees) return;
    const uint64_t pre = T.pre[t];
    if (pre == FF_REFUSED || (pre > 1 && T.madd[t] == 0)) atomicAdd(n_bad, 1u);
}

// ---- every level's records: node g of list l, (tree, node index) as the stored append lists it, in place -> node r = index -
// f_l(n) of its tree's run ----
struct FfLists {
    uint64_t in[FOREST_RAGGED_MAX_DEPTH + 1];
    uint64_t off[FOREST_RAGGED_MAX_DEPTH + 1];
};
__global__ void __launch_bounds__(FF_BLOCK) k_ff_records(const uint64_t* __restrict__ rows, const uint64_t* __restrict__ add_offsets,
                                                         FfTrees T, FfLists L, uint64_t stride, uint4* __restrict__ lists,
                                                         uint32_t* __restrict__ wnode) {
    const unsigned l = blockIdx.y + 1, la = T.la, arity = 1u << la;
    const uint64_t g = (uint64_t)blockIdx.x * FF_BLOCK + threadIdx.x;
    if (g >= L.in[l] || g >= rows[(size_t)l * (T.n_trees + 1) + T.n_trees]) return;
    const size_t at = (size_t)(L.off[l] + g);
    const uint4 rec = lists[at];
    const size_t t = rec.x;
    const uint64_t n = T.nold[t], m = T.madd[t];
    const uint64_t below = floor_shift(n, (l - 1) * la), first = floor_shift(n, l * la) << la;  // f_{l-1}(n), A f_l(n)
    const uint64_t r = u64_of(rec.z, rec.w) - floor_shift(n, l * la);
    const unsigned d = (unsigned)(below - first);  // d_{l-1}(n): children the frontier holds
    // where the tree's run of V_{l-1} starts: in d_add, or in the list of the level below
    const uint64_t base = l == 1 ? add_offsets[t] : rows[(size_t)(l - 1) * (T.n_trees + 1) + t];
    const unsigned all = (1u << arity) - 1u;
    const unsigned mask = r == 0 ? all & ~((1u << d) - 1u) : all;
    const uint64_t run = r == 0 ? base : base + (r << la) - d;
    const uint64_t off = (uint64_t)t * stride + (uint64_t)(l - 1) * (arity - 1);  // row l - 1 of tree t
    lists[at] = make_uint4((unsigned)r, (unsigned)run, (unsigned)off, ((unsigned)(off >> 32) & ((1u << FF_MASK_SHIFT) - 1)) | (mask << FF_MASK_SHIFT));
    wnode[at] = (uint32_t)(ceil_shift(n + m, (l - 1) * la) - first);  // child slot j of the record exists while A r + j is below it
}

// ---- the state, in place: rows 0 .. depth (blockIdx.y), then the root, the count and the digest count (blockIdx.y == depth + 1) ----
__global__ void __launch_bounds__(FF_BLOCK) k_ff_finish(const uint64_t* __restrict__ rows, const uint64_t* __restrict__ add_offsets,
                                                        FfTrees T, FfLists L, uint64_t stride, const Scalar32* __restrict__ add,
                                                        const Scalar32* __restrict__ values, uint64_t* __restrict__ counts,
                                                        Scalar32* __restrict__ frontier, Scalar32* __restrict__ roots,
                                                        unsigned long long* __restrict__ n_hashed) {
    const unsigned l = blockIdx.y, la = T.la, arity = 1u << la;
    const size_t t = (size_t)blockIdx.x * FF_BLOCK + threadIdx.x;
    if (l == T.depth + 1 && t == 0 && n_hashed) {
        unsigned long long hashed = 0;
        for (unsigned k = 1; k <= T.depth; ++k) hashed += rows[(size_t)k * (T.n_trees + 1) + T.n_trees];
        atomicAdd(n_hashed, hashed);
    }
    if (t >= T.n_trees) return;
    const uint64_t m = T.madd[t], n = T.nold[t], nn = n + m;
    if (m == 0) return;  // untouched, root included
    if (l == T.depth + 1) {
        counts[t] = nn;
        if (nn == 1) {  // (no level: the leaf keeps its bytes in row 0, the root is reduced)
            store_scalar(roots + t, load_scalar(add + add_offsets[t]));
            return;
        }
        unsigned top = 1;
        while (ceil_shift(nn, top * la) > 1) ++top;  // D(n') <= depth: n' <= max_leaves
        copy_scalar(reinterpret_cast<uint4*>(roots + t),
                    reinterpret_cast<const uint4*>(values + L.off[top] + rows[(size_t)top * (T.n_trees + 1) + t]));
        return;
    }
    const uint64_t f_old = floor_shift(n, l * la), f_new = floor_shift(nn, l * la);
    const uint64_t up_old = floor_shift(n, (l + 1) * la), up_new = floor_shift(nn, (l + 1) * la);
    // V_l of this tree (read only where the row takes something from it: never for a level the tree does not have)
    const Scalar32* src = l == 0 ? add + add_offsets[t] : values + L.off[l] + rows[(size_t)l * (T.n_trees + 1) + t];
    uint4* row = reinterpret_cast<uint4*>(frontier + (size_t)t * stride + (size_t)l * (arity - 1));
    if (up_new == up_old) {  // the old entries stay; the new final nodes follow them
        const unsigned d = (unsigned)(f_old - (up_old << la)), more = (unsigned)(f_new - f_old);
        for (unsigned k = 0; k < more; ++k) copy_scalar(row + 2 * (d + k), reinterpret_cast<const uint4*>(src + k));
    } else {
        const unsigned d = (unsigned)(f_new - (up_new << la));
        const uint64_t start = (up_new << la) - f_old;
        for (unsigned k = 0; k < arity - 1; ++k) {
            if (k < d)
                copy_scalar(row + 2 * k, reinterpret_cast<const uint4*>(src + start + k));
            else
                store_zero(reinterpret_cast<Scalar32*>(row + 2 * k));
        }
    }
}

// ---- the state of a built forest: rows 0 .. depth (blockIdx.y), then the root and the count (blockIdx.y == depth + 1) ----
__global__ void __launch_bounds__(FF_BLOCK) k_ff_extract(const uint64_t* __restrict__ ntree, const uint64_t* __restrict__ lo,
                                                         const uint64_t* __restrict__ offsets, size_t n_trees, unsigned la, unsigned depth,
                                                         uint64_t stride, const Scalar32* __restrict__ leaves,
                                                         const Scalar32* __restrict__ levels, const Scalar32* __restrict__ roots_forest,
                                                         uint64_t* __restrict__ counts, Scalar32* __restrict__ frontier,
                                                         Scalar32* __restrict__ roots, unsigned* __restrict__ n_bad) {
    const unsigned l = blockIdx.y, arity = 1u << la;
    const size_t t = (size_t)blockIdx.x * FF_BLOCK + threadIdx.x;
    if (t >= n_trees) return;
    const uint64_t n = ntree[t];  // (0: a bad tree — no row of it is read)
    if (l == depth + 1) {
        counts[t] = n;
        if (n == 0) {
            store_zero(roots + t);
            if (n_bad) atomicAdd(n_bad, 1u);
        } else {
            copy_scalar(reinterpret_cast<uint4*>(roots + t), reinterpret_cast<const uint4*>(roots_forest + t));
        }
        return;
    }
    const uint64_t first = floor_shift(n, (l + 1) * la) << la;
    const unsigned d = (unsigned)(floor_shift(n, l * la) - first);
    // (d > 0 at l >= 1 means n >= A^l: the tree has level l)
    const Scalar32* src = nullptr;
    if (d) src = (l == 0 ? leaves + offsets[t] : levels + lo[t] + level_start(n, l, la)) + first;
    uint4* row = reinterpret_cast<uint4*>(frontier + (size_t)t * stride + (size_t)l * (arity - 1));
    for (unsigned k = 0; k < arity - 1; ++k) {
        if (k < d)
            copy_scalar(row + 2 * k, reinterpret_cast<const uint4*>(src + k));
        else
            store_zero(reinterpret_cast<Scalar32*>(row + 2 * k));
    }
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
size_t forest_frontier_stride(unsigned arity, size_t max_leaves) {
    return max_leaves ? (size_t)(forest_ragged_depth(max_leaves, arity) + 1) * (arity - 1) : 0;
}

ForestFrontierPlan forest_frontier_plan(unsigned arity, size_t n_trees, size_t max_leaves, size_t n_add) {
    ForestFrontierPlan p;
    p.arity = arity;
    p.log2a = arity == 4 ? 2 : 1;
    p.depth = forest_ragged_depth(max_leaves, arity);
    p.n_trees = n_trees;
    p.n_add = n_add;
    p.max_leaves = max_leaves;
    p.stride = forest_frontier_stride(arity, max_leaves);
    const size_t growing = n_trees < n_add ? n_trees : n_add;
    for (unsigned l = 1; l <= p.depth; ++l) {
        const unsigned k = l * p.log2a;
        p.in[l] = n_add ? (k >= 64 ? 0 : n_add >> k) + 2 * growing : 0;
        p.list_off[l] = p.records;
        p.records += p.in[l];
    }
    p.tiles = (n_trees + FOREST_APPEND_SCAN_TILE - 1) / FOREST_APPEND_SCAN_TILE;
    const size_t words = 3 * n_trees + (size_t)(p.depth + 1) * (n_trees + 1) + (size_t)(p.depth + 1) * p.tiles;
    p.tree_bytes = (words * 8 + 255) & ~(size_t)255;
    return p;
}

hipError_t launch_forest_frontier_append(const int32_t* tab, const TagArg& tag, const ForestFrontierPlan& p, void* counts, void* frontier,
                                         void* roots, const void* add, const void* add_offsets, void* n_bad, void* n_hashed, void* work,
                                         void* values, const ForestWitnesses* witnesses, hipStream_t st) {
    const size_t T = p.n_trees;
    const bool watched = witnesses && witnesses->k;
    ForestFrontierView view;  // (no tree: every witness is a bad one)
    view.log2a = p.log2a;
    view.depth = p.depth;
    if (T == 0) return watched ? launch_forest_witness_refresh(view, *witnesses, st) : hipSuccess;
    uint64_t* w = static_cast<uint64_t*>(work);
    FfTrees trees;
    trees.nold = w;
    trees.madd = w + T;
    trees.pre = w + 2 * T;
    trees.n_trees = T;
    trees.n_add = p.n_add;
    trees.la = p.log2a;
    trees.depth = p.depth;
    ForestAppendScan scan;
    scan.nold = trees.nold;
    scan.madd = trees.madd;
    scan.rows = w + 3 * T;
    scan.tsum = scan.rows + (size_t)(p.depth + 1) * (T + 1);
    scan.n_trees = T;
    scan.tiles = p.tiles;
    scan.n_add = p.n_add;
    scan.log2a = p.log2a;
    scan.depth = p.depth;
    const uint64_t* rows = scan.rows;
    uint4* lists = reinterpret_cast<uint4*>(static_cast<char*>(work) + p.tree_bytes);
    uint32_t* wnode = reinterpret_cast<uint32_t*>(lists + p.records);
    const uint64_t* aoff = static_cast<const uint64_t*>(add_offsets);
    const dim3 blk(FF_BLOCK), per_tree((unsigned)((T + FF_BLOCK - 1) / FF_BLOCK));

    hipLaunchKernelGGL(k_ff_sizes, per_tree, blk, 0, st, static_cast<const uint64_t*>(counts), aoff, (uint64_t)p.max_leaves, trees);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = forest_append_scan_sum_rule(scan, trees.pre, st);
    if (e != hipSuccess) return e;
    if (n_bad) {
        hipLaunchKernelGGL(k_ff_refused, per_tree, blk, 0, st, trees, static_cast<unsigned*>(n_bad));
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    view.nold = trees.nold;
    view.madd = trees.madd;
    view.rows = rows;
    view.values = values;
    view.add = add;
    view.add_offsets = aoff;
    view.frontier = frontier;
    view.stride = p.stride;
    view.n_trees = T;
    // (nothing to append: the refusals are counted, no tree changes — every m_t is 0, and the witnesses' pass reads the counts alone)
    if (p.n_add == 0) return watched ? launch_forest_witness_refresh(view, *witnesses, st) : hipSuccess;

    FfLists L = {};
    for (unsigned l = 1; l <= p.depth; ++l) {
        L.in[l] = p.in[l];
        L.off[l] = p.list_off[l];
        view.list_off[l] = p.list_off[l];
    }
    if (p.depth) {
        e = forest_append_scan_dirty_lists(scan, p.in, p.list_off, lists, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_ff_records, dim3((unsigned)((p.in[1] + FF_BLOCK - 1) / FF_BLOCK), p.depth), blk, 0, st, rows, aoff, trees, L,
                           (uint64_t)p.stride, lists, wnode);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    Scalar32* vals = static_cast<Scalar32*>(values);
    for (unsigned l = 1; l <= p.depth; ++l) {
        MultiproofDigestList d;
        d.list = lists + p.list_off[l];
        d.count = reinterpret_cast<const unsigned long long*>(rows + (size_t)l * (T + 1) + T);
        d.vals_in = l == 1 ? add : static_cast<const void*>(vals + p.list_off[l - 1]);
        d.vals_out = vals + p.list_off[l];
        d.proof = frontier;
        d.proof_len = T * p.stride;
        d.w_node = wnode + p.list_off[l];
        d.bound = p.in[l];
        e = launch_multiproof_digest_list(tab, tag, p.arity, d, st);
        if (e != hipSuccess) return e;
    }
    if (watched) {  // V_l of every level is in `values`, the frontier still holds the old rows
        e = launch_forest_witness_refresh(view, *witnesses, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ff_finish, dim3(per_tree.x, p.depth + 2), blk, 0, st, rows, aoff, trees, L, (uint64_t)p.stride,
                       static_cast<const Scalar32*>(add), vals, static_cast<uint64_t*>(counts), static_cast<Scalar32*>(frontier),
                       static_cast<Scalar32*>(roots), static_cast<unsigned long long*>(n_hashed));
    return hipGetLastError();
}

hipError_t launch_forest_frontier_extract(unsigned arity, const void* leaves, size_t n_leaves, const void* offsets, size_t n_trees,
                                          size_t max_leaves_forest, const void* levels, const void* roots_forest, size_t max_leaves,
                                          void* counts, void* frontier, void* roots, void* n_bad, void* meta, hipStream_t st) {
    if (n_trees == 0) return hipSuccess;
    const uint64_t *ntree = nullptr, *lo = nullptr;
    hipError_t e = launch_forest_ragged_index(arity, offsets, n_trees, n_leaves, max_leaves_forest, meta, &ntree, &lo, st);
    if (e != hipSuccess) return e;
    const unsigned depth = forest_ragged_depth(max_leaves, arity);
    hipLaunchKernelGGL(k_ff_extract, dim3((unsigned)((n_trees + FF_BLOCK - 1) / FF_BLOCK), depth + 2), dim3(FF_BLOCK), 0, st, ntree, lo,
                       static_cast<const uint64_t*>(offsets), n_trees, arity == 4 ? 2u : 1u, depth,
                       (uint64_t)forest_frontier_stride(arity, max_leaves), static_cast<const Scalar32*>(leaves),
                       static_cast<const Scalar32*>(levels), static_cast<const Scalar32*>(roots_forest), static_cast<uint64_t*>(counts),
                       static_cast<Scalar32*>(frontier), static_cast<Scalar32*>(roots), static_cast<unsigned*>(n_bad));
    return hipGetLastError();
}

}  // namespace p252
