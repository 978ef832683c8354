// forest_append.hip — leaves appended to the trees of a built forest of trees of DIFFERENT sizes (forest_ragged.hip, tree-major
// levels), written as a new compact forest, for both arities (p252_merkle{4,2}_forest_ragged_append_device_into) — and the same after
// every tree was cut to its first k_t <= n_t leaves (p252_merkle{4,2}_forest_ragged_resize_device_into: a rollback, a reorg, a prune;
// the new forest may also have fewer trees than the old one).  A tree's size fixes its level layout, so a tree that changes moves;
// but of a tree of n leaves that keeps its first k and receives m more, node j of level l is unchanged iff j < floor(k / a^l), and
// it sits at the same (l, j) in the old tree (with k == n and m == 0 every node is unchanged — the last, partly filled parent too:
// floor(n / a^l) is NOT the old level's width).  Every other node of the new tree has a new leaf or the cut below it.  The append is
// the k == n case.  So the call MOVES the clean nodes and hashes only the dirty ones, sum over l >= 1 of ceil((k + m) / a^l) -
// floor(k / a^l) per tree that changes — with m == 0 at most one node per level:
//   k_fa_sizes        per tree of the new forest: n_t of the old forest's index (0: a bad tree, or none), the kept count k_t =
//                     min(keep[t], n_t) (no keep array: n_t) and the append m_t, or "refused" (decreasing add offsets, a range past
//                     n_add, k_t + m_t > max_leaves_new); the cut holds for a refused append too
//   k_fa_tile_sums / k_fa_scan_tiles / k_fa_scan_apply   the unit's exclusive device-wide scan (tiles of 2,048 trees), three uses:
//                     SUM  over m_t: an append that takes the running sum of the appends before it past n_add is refused as well
//                          (that only happens when ranges overlap behind decreasing offsets; it keeps the new leaves within
//                          n_leaves + n_add and every dirty list within the host's bound); a refused append counts as m_t = 0;
//                          *n_bad grows once per tree that is refused or empty in the new forest, whose root is written as zero
//                     OFFS over k_t + m_t: d_offsets_new
//                     DIRTY over every level's dirty count at once (gridDim.y): row l = where tree t's records start in list l
//   (launch_forest_ragged_index on d_offsets_new: the new forest's leaf counts and block starts are the build's own)
//   k_fa_tile_first   per 512-scalar tile of the new leaves / of the new levels: the tree that holds its first scalar, so a
//                     relocation lane looks for its tree between the first trees of its tile and of the next (no probe inside a
//                     large tree, <= 9 over trees of one leaf)
//   k_fa_move_leaves  one lane per 16-byte half of four new leaves: leaf i < k_t from the tree's old leaves, the others from d_add
//   k_fa_move_nodes   one lane per 16-byte half of four slots of the new levels: a clean node comes from its old block (both
//                     addresses by the closed forms of forest_node.hpp), a dirty slot is left to the digests
//   k_fa_roots        the roots no digest writes: zero (an empty tree), the reduced leaf (one leaf, as k_fu_scatter: a tree cut to one
//                     leaf too), the top of the block (an unchanged tree, and a tree cut to a whole power of the arity)
//   k_fa_expand       every level at once (gridDim.y): record g of list l = (tree, floor(k / a^l) + g - row_l[t]), in the 16-byte
//                     format of forest_update.hip; the list's count is row_l[n_trees]
// then launch_forest_digest_list (forest_update.hip) per level: level l reads level l - 1 of the NEW forest only — moved or hashed
// by an earlier launch.  No kernel here hashes.  forest_append_scan_sum_rule / forest_append_scan_dirty_lists run the SUM scan and
// the DIRTY scans with k_fa_expand on per-tree words their caller made: forest_frontier.hip, which appends to trees kept as frontiers.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_append.h"
#include "forest_node.hpp"
#include "forest_update.h"

namespace p252 {

namespace {

constexpr unsigned FA_BLOCK = 256;
constexpr unsigned FA_ITEMS = FOREST_APPEND_SCAN_TILE / FA_BLOCK;  // trees per thread of a scan block
constexpr unsigned FA_MOVE = 2 * FOREST_APPEND_MOVE_TILE / FA_BLOCK;  // 16-byte halves per lane of a relocation block
constexpr uint64_t FA_REFUSED = FOREST_APPEND_REFUSED;
enum { FA_SUM = 0, FA_OFFS = 1, FA_DIRTY = 2 };

struct FaTrees {
    uint64_t* nold;  // n_t in the old forest
    uint64_t* keep;  // k_t <= n_t: the old leaves the tree keeps (an append: n_t)
    uint64_t* madd;  // m_t (FA_REFUSED between k_fa_sizes and the SUM scan)
    size_t n_trees;
    uint64_t n_add;
    unsigned la;
};

__device__ __forceinline__ uint64_t floor_shift(uint64_t n, unsigned k) { return k >= 64 ? 0ull : n >> k; }

// dirty nodes of level l of a tree of n leaves that keeps its first k and receives m more
__device__ __forceinline__ uint64_t dirty_nodes(uint64_t n, uint64_t k, uint64_t m, unsigned l, unsigned la) {
    if (m == 0 && k == n) return 0;
    const uint64_t w = level_nodes(k + m, l, la);
    return w ? w - floor_shift(k, l * la) : 0ull;
}

template <int MODE>
__device__ __forceinline__ uint64_t scan_value(const FaTrees& T, size_t t, unsigned l) {
    const uint64_t m = T.madd[t];
    if (MODE == FA_SUM) return m == FA_REFUSED ? 0ull : m;
    if (MODE == FA_OFFS) return T.keep[t] + m;
    return dirty_nodes(T.nold[t], T.keep[t], m, l, T.la);
}

}  // namespace

// ---- per tree: the old leaf count, the kept count (keep_in null: every tree whole) and the append ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_sizes(const uint64_t* __restrict__ ntree_old, size_t n_trees_old,
                                                       const uint64_t* __restrict__ keep_in, const uint64_t* __restrict__ add_offsets,
                                                       uint64_t max_leaves_new, FaTrees T) {
    const size_t t = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    if (t >= T.n_trees) return;
    const uint64_t n = t < n_trees_old ? ntree_old[t] : 0ull;  // (n <= max_leaves <= max_leaves_new: api.cpp)
    const uint64_t want = keep_in ? keep_in[t] : n;
    const uint64_t k = want < n ? want : n;  // (the truncation is always valid: it holds for a refused append too)
    const uint64_t lo = add_offsets[t], hi = add_offsets[t + 1];
    const uint64_t m = hi - lo;
    const bool ok = hi >= lo && hi <= T.n_add && m <= max_leaves_new - k;
    T.nold[t] = n;
    T.keep[t] = k;
    T.madd[t] = ok ? m : FA_REFUSED;
}

// ---- the scan: tiles of FOREST_APPEND_SCAN_TILE trees; DIRTY scans level blockIdx.y + 1 into row blockIdx.y + 1 ----
template <int MODE>
__global__ void __launch_bounds__(FA_BLOCK) k_fa_tile_sums(FaTrees T, uint64_t* __restrict__ tsum) {
    const unsigned l = blockIdx.y + 1;
    const size_t t0 = (size_t)blockIdx.x * FOREST_APPEND_SCAN_TILE + (size_t)threadIdx.x * FA_ITEMS;
    uint64_t sum = 0;
#pragma unroll 1
    for (unsigned k = 0; k < FA_ITEMS; ++k)
        if (t0 + k < T.n_trees) sum += scan_value<MODE>(T, t0 + k, l);
    uint64_t total;
    (void)block_exclusive<FA_BLOCK>(sum, &total);
    if (threadIdx.x == 0) tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one block per row (SUM, OFFS, one DIRTY row per level): the tile sums of the row -> their exclusive scan, in place (scan_tile_row of
// blockops.hpp: the second trip of its loop starts past FA_BLOCK * FOREST_APPEND_SCAN_TILE = 524,288 new trees)
__global__ void __launch_bounds__(FA_BLOCK) k_fa_scan_tiles(uint64_t* __restrict__ tsum, size_t tiles) {
    scan_tile_row<FA_BLOCK>(tsum + (size_t)blockIdx.x * tiles, tiles);
}

// SUM: the sum rule, m_t settled, the bad trees counted and their roots zeroed.  OFFS: out = d_offsets_new (n_trees + 1).
// DIRTY: out = the rows (n_trees + 1 each).
template <int MODE>
__global__ void __launch_bounds__(FA_BLOCK) k_fa_scan_apply(FaTrees T, const uint64_t* __restrict__ tsum, uint64_t* __restrict__ out,
                                                            Scalar32* __restrict__ roots, unsigned* __restrict__ n_bad) {
    const unsigned l = blockIdx.y + 1;
    const size_t t0 = (size_t)blockIdx.x * FOREST_APPEND_SCAN_TILE + (size_t)threadIdx.x * FA_ITEMS;
    uint64_t sum = 0;
#pragma unroll 1
    for (unsigned k = 0; k < FA_ITEMS; ++k)
        if (t0 + k < T.n_trees) sum += scan_value<MODE>(T, t0 + k, l);
    uint64_t total;
    uint64_t run = tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive<FA_BLOCK>(sum, &total);
    uint64_t* row = MODE == FA_DIRTY ? out + (size_t)l * (T.n_trees + 1) : out;
#pragma unroll 1
    for (unsigned k = 0; k < FA_ITEMS; ++k) {
        const size_t t = t0 + k;
        if (t >= T.n_trees) break;
        const uint64_t v = scan_value<MODE>(T, t, l);
        if (MODE == FA_SUM) {
            // (run <= n_trees * n_add < 2^63: api.cpp refuses larger)
            const bool refused = T.madd[t] == FA_REFUSED || (v != 0 && (run > T.n_add || v > T.n_add - run));  // (nothing appended: nothing to refuse)
            const uint64_t m = refused ? 0ull : v;
            T.madd[t] = m;
            const bool empty = T.keep[t] + m == 0;
            if (empty) store_zero(roots + t);
            if ((refused || empty) && n_bad) atomicAdd(n_bad, 1u);
        } else {
            row[t] = run;
            if (t == T.n_trees - 1) row[T.n_trees] = run + v;
        }
        run += v;
    }
}

// ---- the tree that holds scalar FOREST_APPEND_MOVE_TILE * b of B (n_trees + 1 starts): the largest t < n_trees with B[t] <= it ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_tile_first(const uint64_t* __restrict__ B, size_t n_trees, size_t entries,
                                                            uint64_t* __restrict__ first) {
    const size_t b = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    if (b >= entries) return;
    first[b] = last_at_or_below(B, 0, n_trees - 1, (uint64_t)b * FOREST_APPEND_MOVE_TILE);  // (B[0] = 0)
}

// ---- the leaves: each tree's kept ones, then its appended ones ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_move_leaves(const uint64_t* __restrict__ off_new, const uint64_t* __restrict__ first,
                                                             const uint64_t* __restrict__ off_old, const uint64_t* __restrict__ add_offsets,
                                                             FaTrees T, const uint4* __restrict__ leaves, const uint4* __restrict__ add,
                                                             uint4* __restrict__ leaves_new) {
    const uint64_t total = off_new[T.n_trees];
    const size_t lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
#pragma unroll
    for (unsigned u = 0; u < FA_MOVE; ++u) {
        const uint64_t h = ((uint64_t)blockIdx.x * FA_MOVE + u) * FA_BLOCK + threadIdx.x;  // the 16-byte half
        const uint64_t j = h >> 1;
        if (j >= total) return;
        const size_t t = last_at_or_below(off_new, lo, hi, j);
        const uint64_t i = j - off_new[t], k = T.keep[t];
        const uint4* src = i < k ? leaves + 2 * (off_old[t] + i) : add + 2 * (add_offsets[t] + (i - k));
        leaves_new[h] = src[h & 1];
    }
}

// ---- the clean nodes: from the tree's old block to its new one ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_move_nodes(const uint64_t* __restrict__ lo_new, const uint64_t* __restrict__ first,
                                                            const uint64_t* __restrict__ lo_old, FaTrees T, const uint4* __restrict__ levels,
                                                            uint4* __restrict__ levels_new) {
    const uint64_t total = lo_new[T.n_trees];
    const size_t lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
#pragma unroll
    for (unsigned u = 0; u < FA_MOVE; ++u) {
        const uint64_t h = ((uint64_t)blockIdx.x * FA_MOVE + u) * FA_BLOCK + threadIdx.x;
        const uint64_t s = h >> 1;
        if (s >= total) return;
        const size_t t = last_at_or_below(lo_new, lo, hi, s);
        const uint64_t p = s - lo_new[t], n = T.nold[t], k = T.keep[t], m = T.madd[t];
        uint64_t from = p;  // (k == n, m == 0: the same tree, the same layout)
        if (m != 0 || k != n) {
            // the level of slot p of the new block (of k + m leaves), and its place in it
            uint64_t start = 0, w = ceil_shift(k + m, T.la);
            unsigned l = 1;
#pragma unroll 1
            while (p >= start + w && w > 1) {  // (w == 1: the top; the index and n + m agree, so p never lies past it)
                start += w;
                ++l;
                w = ceil_shift(k + m, l * T.la);
            }
            const uint64_t j = p - start;
            if (j >= floor_shift(k, l * T.la)) continue;  // dirty: a digest writes it
            from = level_start(n, l, T.la) + j;
        }
        levels_new[h] = levels[2 * (lo_old[t] + from) + (h & 1)];
    }
}

// ---- the roots no digest writes (an empty tree's is zero already: the SUM scan) ----
__global__ void __launch_bounds__(FA_BLOCK) k_fa_roots(const uint64_t* __restrict__ off_new, const uint64_t* __restrict__ lo_new, FaTrees T,
                                                       const Scalar32* __restrict__ leaves_new, const Scalar32* __restrict__ levels_new,
                                                       Scalar32* __restrict__ roots) {
    const size_t t = (size_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    if (t >= T.n_trees) return;
    const uint64_t m = T.madd[t], k = T.keep[t], n = k + m;
    // the top node is clean in an unchanged tree, and in a tree cut to a whole power of the arity: its old subtree of that height
    const bool top_clean = m == 0 && (k == T.nold[t] || ((k & (k - 1)) == 0 && (unsigned)(__ffsll((long long)k) - 1) % T.la == 0));
    if (n == 1) {  // (the leaf keeps its bytes; the root is reduced, as the forest's build writes it: a tree cut to one leaf too)
        store_scalar(roots + t, load_scalar(leaves_new + off_new[t]));
    } else if (n > 1 && top_clean) {  // no digest writes it: the last scalar of its block, moved there
        const uint4* src = reinterpret_cast<const uint4*>(levels_new + lo_new[t + 1] - 1);
        uint4* dst = reinterpret_cast<uint4*>(roots + t);
        dst[0] = src[0];
        dst[1] = src[1];
    }
}

// ---- every level's dirty list ----
struct FaLists {
    uint64_t in[FOREST_RAGGED_MAX_DEPTH + 1];
    uint64_t off[FOREST_RAGGED_MAX_DEPTH + 1];
};
__global__ void __launch_bounds__(FA_BLOCK) k_fa_expand(const uint64_t* __restrict__ rows, FaTrees T, FaLists L, uint4* __restrict__ lists) {
    const unsigned l = blockIdx.y + 1;
    const uint64_t g = (uint64_t)blockIdx.x * FA_BLOCK + threadIdx.x;
    const uint64_t* __restrict__ row = rows + (size_t)l * (T.n_trees + 1);
    if (g >= L.in[l] || g >= row[T.n_trees]) return;
    const size_t t = last_at_or_below(row, 0, T.n_trees - 1, g);
    const uint64_t i = floor_shift(T.keep[t], l * T.la) + (g - row[t]);
    lists[L.off[l] + g] = record((uint32_t)t, i);
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
ForestAppendPlan forest_append_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t n_add, size_t n_trees_new,
                                    size_t max_leaves_new, size_t leaves_cap) {
    ForestAppendPlan p;
    const size_t N = n_leaves + n_add, T = n_trees_new;
    const ForestRaggedPlan fr = forest_ragged_plan(arity, N, T, max_leaves_new, true);
    p.arity = arity;
    p.log2a = fr.log2a;
    p.depth = fr.depth;
    p.n_trees_old = n_trees;
    p.n_trees = T;
    p.n_leaves_old = n_leaves;
    p.n_add = n_add;
    p.leaves = N;
    p.max_leaves_old = max_leaves;
    p.max_leaves = max_leaves_new;
    p.leaves_cap = leaves_cap;
    p.nodes = N / (arity - 1) + T * p.depth;
    size_t records = 0;
    for (unsigned l = 1; l <= p.depth; ++l) {
        const size_t dirty = (n_add >> (l * p.log2a)) + 2 * T;
        p.in[l] = dirty < fr.bound[l] ? dirty : fr.bound[l];
        p.list_off[l] = records;
        records += p.in[l];
    }
    p.tiles = (T + FOREST_APPEND_SCAN_TILE - 1) / FOREST_APPEND_SCAN_TILE;
    p.leaf_tiles = (N + FOREST_APPEND_MOVE_TILE - 1) / FOREST_APPEND_MOVE_TILE;
    p.node_tiles = (p.nodes + FOREST_APPEND_MOVE_TILE - 1) / FOREST_APPEND_MOVE_TILE;
    p.index_old_bytes = forest_ragged_index_bytes(n_trees);
    p.index_new_bytes = forest_ragged_index_bytes(T);
    // n_t, k_t and m_t, the rows (row 0 unused), the scans' tile sums, the two first-tree rows
    const size_t words = 3 * T + (size_t)(p.depth + 1) * (T + 1) + (size_t)(p.depth + 1) * p.tiles + p.leaf_tiles + 1 + p.node_tiles + 1;
    p.work_bytes = (words * 8 + 255) & ~(size_t)255;
    p.list_bytes = records * sizeof(uint4);
    return p;
}

hipError_t launch_forest_append(const int32_t* tab, const TagArg& tag, const ForestAppendPlan& p, const void* leaves, const void* offsets,
                                const void* levels, const void* keep, const void* add, const void* add_offsets, void* leaves_new,
                                void* offsets_new, void* levels_new, void* roots, void* n_bad, void* n_hashed, void* meta, void* lists,
                                hipStream_t st) {
    const size_t T = p.n_trees;
    if (T == 0) return hipSuccess;
    char* base = static_cast<char*>(meta);
    const uint64_t *ntree_old = nullptr, *lo_old = nullptr, *ntree_new = nullptr, *lo_new = nullptr;
    hipError_t e = launch_forest_ragged_index(p.arity, offsets, p.n_trees_old, p.n_leaves_old, p.max_leaves_old, base, &ntree_old, &lo_old, st);
    if (e != hipSuccess) return e;
    uint64_t* w = reinterpret_cast<uint64_t*>(base + p.index_old_bytes + p.index_new_bytes);
    FaTrees trees;
    trees.nold = w;
    trees.keep = w + T;
    trees.madd = w + 2 * T;
    trees.n_trees = T;
    trees.n_add = p.n_add;
    trees.la = p.log2a;
    uint64_t* rows = w + 3 * T;
    uint64_t* tsum = rows + (size_t)(p.depth + 1) * (T + 1);
    uint64_t* first_leaf = tsum + (size_t)(p.depth + 1) * p.tiles;
    uint64_t* first_node = first_leaf + p.leaf_tiles + 1;
    const uint64_t* aoff = static_cast<const uint64_t*>(add_offsets);
    uint64_t* off_new = static_cast<uint64_t*>(offsets_new);
    Scalar32* rt = static_cast<Scalar32*>(roots);
    const dim3 blk(FA_BLOCK), per_tree((unsigned)((T + FA_BLOCK - 1) / FA_BLOCK)), tiles((unsigned)p.tiles);

    hipLaunchKernelGGL(k_fa_sizes, per_tree, blk, 0, st, ntree_old, p.n_trees_old, static_cast<const uint64_t*>(keep), aoff,
                       (uint64_t)p.max_leaves, trees);
    hipLaunchKernelGGL(k_fa_tile_sums<FA_SUM>, tiles, blk, 0, st, trees, tsum);
    hipLaunchKernelGGL(k_fa_scan_tiles, dim3(1), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fa_scan_apply<FA_SUM>, tiles, blk, 0, st, trees, tsum, (uint64_t*)nullptr, rt, static_cast<unsigned*>(n_bad));
    hipLaunchKernelGGL(k_fa_tile_sums<FA_OFFS>, tiles, blk, 0, st, trees, tsum);
    hipLaunchKernelGGL(k_fa_scan_tiles, dim3(1), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fa_scan_apply<FA_OFFS>, tiles, blk, 0, st, trees, tsum, off_new, rt, (unsigned*)nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the new forest's index: the build's own validation and block starts, on the offsets just written
    e = launch_forest_ragged_index(p.arity, off_new, T, p.leaves_cap, p.max_leaves, base + p.index_old_bytes, &ntree_new, &lo_new, st);
    if (e != hipSuccess) return e;

    if (p.leaves) {
        hipLaunchKernelGGL(k_fa_tile_first, dim3((unsigned)((p.leaf_tiles + 1 + FA_BLOCK - 1) / FA_BLOCK)), blk, 0, st, off_new, T,
                           p.leaf_tiles + 1, first_leaf);
        hipLaunchKernelGGL(k_fa_move_leaves, dim3((unsigned)p.leaf_tiles), blk, 0, st, off_new, first_leaf, static_cast<const uint64_t*>(offsets),
                           aoff, trees, static_cast<const uint4*>(leaves), static_cast<const uint4*>(add), static_cast<uint4*>(leaves_new));
    }
    if (p.depth && p.nodes) {
        hipLaunchKernelGGL(k_fa_tile_first, dim3((unsigned)((p.node_tiles + 1 + FA_BLOCK - 1) / FA_BLOCK)), blk, 0, st, lo_new, T,
                           p.node_tiles + 1, first_node);
        hipLaunchKernelGGL(k_fa_move_nodes, dim3((unsigned)p.node_tiles), blk, 0, st, lo_new, first_node, lo_old, trees,
                           static_cast<const uint4*>(levels), static_cast<uint4*>(levels_new));
    }
    hipLaunchKernelGGL(k_fa_roots, per_tree, blk, 0, st, off_new, lo_new, trees, static_cast<const Scalar32*>(leaves_new),
                       static_cast<const Scalar32*>(levels_new), rt);
    e = hipGetLastError();
    if (e != hipSuccess || p.depth == 0 || (p.n_add == 0 && !keep)) return e;  // (nothing appended, nothing cut: a compaction copy, every node clean)

    FaLists L = {};
    for (unsigned l = 1; l <= p.depth; ++l) {
        L.in[l] = p.in[l];
        L.off[l] = p.list_off[l];
    }
    hipLaunchKernelGGL(k_fa_tile_sums<FA_DIRTY>, dim3((unsigned)p.tiles, p.depth), blk, 0, st, trees, tsum);
    hipLaunchKernelGGL(k_fa_scan_tiles, dim3(p.depth), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fa_scan_apply<FA_DIRTY>, dim3((unsigned)p.tiles, p.depth), blk, 0, st, trees, tsum, rows, rt, (unsigned*)nullptr);
    hipLaunchKernelGGL(k_fa_expand, dim3((unsigned)((p.in[1] + FA_BLOCK - 1) / FA_BLOCK), p.depth), blk, 0, st, rows, trees, L,
                       static_cast<uint4*>(lists));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (unsigned l = 1; l <= p.depth; ++l) {
        ForestDigestList d;
        d.list = static_cast<const uint4*>(lists) + p.list_off[l];
        d.count = reinterpret_cast<const unsigned long long*>(rows + (size_t)l * (T + 1) + T);
        d.bound = p.in[l];
        d.ntree = ntree_new;
        d.lo = lo_new;
        d.offsets = off_new;
        d.leaves = leaves_new;
        d.levels = levels_new;
        d.roots = roots;
        d.n_hashed = n_hashed;
        d.level = l;
        e = launch_forest_digest_list(tab, tag, p.arity, p.log2a, d, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- the same scans over per-tree words that the caller made (forest_frontier.hip): no old forest, every tree keeps its n_t leaves ----
namespace {
FaTrees scan_trees(const ForestAppendScan& s, const uint64_t* keep) {
    FaTrees trees;
    trees.nold = s.nold;
    trees.keep = const_cast<uint64_t*>(keep);  // (read only by the scans)
    trees.madd = s.madd;
    trees.n_trees = s.n_trees;
    trees.n_add = s.n_add;
    trees.la = s.log2a;
    return trees;
}
}  // namespace

hipError_t forest_append_scan_sum_rule(const ForestAppendScan& s, const uint64_t* never_zero, hipStream_t st) {
    const FaTrees trees = scan_trees(s, never_zero);
    const dim3 blk(FA_BLOCK), tiles((unsigned)s.tiles);
    hipLaunchKernelGGL(k_fa_tile_sums<FA_SUM>, tiles, blk, 0, st, trees, s.tsum);
    hipLaunchKernelGGL(k_fa_scan_tiles, dim3(1), blk, 0, st, s.tsum, s.tiles);
    // (keep + m is never zero: no tree is empty, no root is written, and without a counter nothing is counted)
    hipLaunchKernelGGL(k_fa_scan_apply<FA_SUM>, tiles, blk, 0, st, trees, s.tsum, (uint64_t*)nullptr, (Scalar32*)nullptr, (unsigned*)nullptr);
    return hipGetLastError();
}

hipError_t forest_append_scan_dirty_lists(const ForestAppendScan& s, const size_t* in, const size_t* list_off, void* lists, hipStream_t st) {
    if (s.depth == 0) return hipSuccess;
    const FaTrees trees = scan_trees(s, s.nold);
    FaLists L = {};
    for (unsigned l = 1; l <= s.depth; ++l) {
        L.in[l] = in[l];
        L.off[l] = list_off[l];
    }
    const dim3 blk(FA_BLOCK);
    hipLaunchKernelGGL(k_fa_tile_sums<FA_DIRTY>, dim3((unsigned)s.tiles, s.depth), blk, 0, st, trees, s.tsum);
    hipLaunchKernelGGL(k_fa_scan_tiles, dim3(s.depth), blk, 0, st, s.tsum, s.tiles);
    hipLaunchKernelGGL(k_fa_scan_apply<FA_DIRTY>, dim3((unsigned)s.tiles, s.depth), blk, 0, st, trees, s.tsum, s.rows, (Scalar32*)nullptr, (unsigned*)nullptr);
    hipLaunchKernelGGL(k_fa_expand, dim3((unsigned)((in[1] + FA_BLOCK - 1) / FA_BLOCK), s.depth), blk, 0, st, s.rows, trees, L, static_cast<uint4*>(lists));
    return hipGetLastError();
}

}  // namespace p252
