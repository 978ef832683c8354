// forest_ragged.hip — a forest of Merkle trees of DIFFERENT sizes in one call (p252_merkle{4,2}_forest_ragged*).  Tree t =
// leaves[offsets[t] .. offsets[t+1]), n_t leaves; each tree is what p252_merkle{4,2}_tree builds: level l has
// s_l(t) = ceil(n_t / a^l) nodes while level l-1 had more than one, missing children are the zero scalar, a single leaf is its
// own root.
//
// Why new digest kernels: a level's node count depends on the tree sizes, and in the device form those live on the device, so
// launch_merkle4 (an exact count, children contiguous and aligned to the arity) cannot be used.  Instead each level is ONE
// launch over the concatenation of all trees' nodes at that level:
//   k_fr_prep          per tree: n_t, or 0 for a bad tree (empty, longer than max_leaves, decreasing offsets, past n_leaves)
//   k_fr_tile_sums / k_fr_scan_tiles / k_fr_scan_apply   an exclusive device-wide scan, three passes (tiles of 2,048 trees),
//                      over several rows at once (gridDim.y).  First over n_t alone: a tree whose n_t takes the running sum of
//                      the leaf counts before it past n_leaves is bad as well — that only happens when trees overlap behind
//                      decreasing offsets, and it is what keeps every level within the host's bound n_leaves / a^l + n_trees.
//                      The same pass writes the roots of bad trees (zero); k_fr_prep wrote those of single-leaf trees (the
//                      leaf, reduced).  Then over
//                      every level l at once: C_l = the scan of s_l (row l), and LO = the scan of levels_len(n_t) (row 0,
//                      only when the caller's d_levels is written).
//   k_fr_rows_tile_sums / k_fr_rows_apply   the same three-pass scan (with k_fr_scan_tiles between them) over rows of values that
//                      ANOTHER unit wrote — launch_forest_scan_rows: forest_range.hip's per-level node counts of its runs
//   k_fr_block_first   per level and 256-node block b: the tree that holds node 256 b — so a digest lane looks for its tree
//                      only between the first trees of its block and of the next one (<= 8 probes on a dense level)
//   k_fr_digest / k_fr_digest_coop   lane (group of 8 lanes) g hashes node g of level l: t with C_l[t] <= g < C_l[t+1],
//                      i = g - C_l[t]; children a i .. a i + a - 1 of tree t's level l-1 (zero at or past s_{l-1}(t)).
//                      Level 0 is the tree's leaves; level l-1 >= 1 is read from the tree's block of d_levels (tree-major,
//                      closed-form offset) or from the level-major scratch at C_{l-1}[t].  A node that is its tree's only
//                      node at level l is its root: in the level-major mode it goes to d_roots[t] instead of the scratch; in
//                      the tree-major mode k_fr_roots_from_levels copies it from the end of the tree's block after the last
//                      level (one output pointer per lane: the lane groups then hold their 256 VGPRs without AGPR spills).
// The permutation is the library's: hades_permute<0x02u, true> with the hoisted tag S-box (the k_merkle4 build, 3 waves per SIMD),
// written out in k_fr_digest and again in k_fu_digest (through a shared function both come out with other instruction streams:
// profiles/forest_kernels_refactor.txt), and hades_permute_coop<8> for levels that cannot fill the chip (the coop8 rule of
// kernels.h) — node_digest_coop of forest_node.hpp, which holds what the three forest files share.
// The unit also holds the SELECT (p252_merkle{4,2}_forest_ragged_select_device_into): trees of built forests gathered into a new forest
// with no digest — k_fr_sel_*, data movement and bookkeeping only, described above its kernels below.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_node.hpp"
#include "forest_ragged.h"
#include "hades29.hpp"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FR_BLOCK = 256;
constexpr unsigned FR_ITEMS = 8;  // trees per thread of a scan block
constexpr unsigned FR_TILE = FR_BLOCK * FR_ITEMS;
constexpr unsigned FR_ROW_LEAVES = 0xffffffffu;  // scan row of the leaf counts n_t themselves

__device__ __forceinline__ uint64_t row_value(const uint64_t* __restrict__ ntree, size_t t, unsigned row, unsigned la) {
    const uint64_t n = ntree[t];
    if (row == FR_ROW_LEAVES) return n;
    return row == 0 ? levels_len_dev(n, la) : level_nodes(n, row, la);
}

}  // namespace

// ---- validation ----
// (with `roots`: the root of a single-leaf tree, its leaf REDUCED as every output is — what k_path_ragged gives for the tree's only
// opening, of depth 0; the scan's first pass overwrites it with zero if the sum rule finds the tree bad after all)
__global__ void __launch_bounds__(FR_BLOCK) k_fr_prep(const uint64_t* __restrict__ offsets, size_t n_trees, uint64_t n_leaves,
                                                      uint64_t max_leaves, uint64_t* __restrict__ ntree,
                                                      const Scalar32* __restrict__ leaves, Scalar32* __restrict__ roots) {
    const size_t t = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (t >= n_trees) return;
    const uint64_t lo = offsets[t], hi = offsets[t + 1];
    const uint64_t n = hi - lo;
    const bool good = hi >= lo && n >= 1 && n <= max_leaves && hi <= n_leaves;
    ntree[t] = good ? n : 0;
    if (good && n == 1 && roots) store_scalar(roots + t, load_scalar(leaves + lo));
}

// ---- the scan: rows row0 + blockIdx.y (row0 == FR_ROW_LEAVES: that one row), tiles of FR_TILE trees ----
__device__ __forceinline__ unsigned scan_row(unsigned row0) { return row0 == FR_ROW_LEAVES ? row0 : row0 + blockIdx.y; }

__global__ void __launch_bounds__(FR_BLOCK) k_fr_tile_sums(const uint64_t* __restrict__ ntree, size_t n_trees, unsigned row0, unsigned la,
                                                           uint64_t* __restrict__ tsum) {
    const unsigned row = scan_row(row0);
    const size_t t0 = (size_t)blockIdx.x * FR_TILE + (size_t)threadIdx.x * FR_ITEMS;
    uint64_t sum = 0;
#pragma unroll 1
    for (unsigned k = 0; k < FR_ITEMS; ++k)
        if (t0 + k < n_trees) sum += row_value(ntree, t0 + k, row, la);
    uint64_t total;
    (void)block_exclusive<FR_BLOCK>(sum, &total);
    if (threadIdx.x == 0) tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one block per row: the tile sums of the row -> their exclusive scan, in place (scan_tile_row of blockops.hpp: the second trip of its
// loop starts past FR_BLOCK * FR_TILE = 524,288 trees)
__global__ void __launch_bounds__(FR_BLOCK) k_fr_scan_tiles(uint64_t* __restrict__ tsum, size_t tiles) {
    scan_tile_row<FR_BLOCK>(tsum + (size_t)blockIdx.x * tiles, tiles);
}

// FIRST (the leaf-count row): the sum rule above, then the roots of bad trees (zero).  Otherwise: C[row][t] for every
// tree and C[row][n_trees] = the row's total.
template <bool FIRST>
__global__ void __launch_bounds__(FR_BLOCK) k_fr_scan_apply(uint64_t* __restrict__ ntree, size_t n_trees, unsigned row0, unsigned la,
                                                            const uint64_t* __restrict__ tsum, uint64_t* __restrict__ C,
                                                            uint64_t n_leaves, const uint64_t* __restrict__ offsets,
                                                            const Scalar32* __restrict__ leaves, Scalar32* __restrict__ roots,
                                                            unsigned* __restrict__ n_bad) {
    const unsigned row = scan_row(row0);
    const size_t t0 = (size_t)blockIdx.x * FR_TILE + (size_t)threadIdx.x * FR_ITEMS;
    uint64_t v[FR_ITEMS], sum = 0;
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        v[k] = t0 + k < n_trees ? row_value(ntree, t0 + k, row, la) : 0ull;
        sum += v[k];
    }
    uint64_t total;
    uint64_t run = tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive<FR_BLOCK>(sum, &total);
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        const size_t t = t0 + k;
        if (t >= n_trees) break;
        if (FIRST) {
            uint64_t n = v[k];
            if (run > n_leaves || n > n_leaves - run) {  // (run <= n_trees * max_leaves < 2^63: api.cpp refuses larger)
                n = 0;
                ntree[t] = 0;
            }
            if (!roots) {  // (the index alone: launch_forest_ragged_index)
            } else if (n == 0) {
                store_zero(roots + t);
                if (n_bad) atomicAdd(n_bad, 1u);
            }  // (n == 1: k_fr_prep wrote the root)
        } else {
            uint64_t* Crow = C + (size_t)row * (n_trees + 1);
            Crow[t] = run;
            if (t == n_trees - 1) Crow[n_trees] = run + v[k];
        }
        run += v[k];
    }
}

// ---- the same scan over rows of values that a caller wrote (launch_forest_scan_rows): row blockIdx.y of v, n values a row, in place ----
__global__ void __launch_bounds__(FR_BLOCK) k_fr_rows_tile_sums(const uint64_t* __restrict__ v, size_t n, uint64_t* __restrict__ tsum) {
    const uint64_t* __restrict__ row = v + (size_t)blockIdx.y * n;
    const size_t t0 = (size_t)blockIdx.x * FR_TILE + (size_t)threadIdx.x * FR_ITEMS;
    uint64_t sum = 0;
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k)
        if (t0 + k < n) sum += row[t0 + k];
    uint64_t total;
    (void)block_exclusive<FR_BLOCK>(sum, &total);
    if (threadIdx.x == 0) tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// v[row][i] becomes the sum of the row's values before i, totals[row] the row's sum
__global__ void __launch_bounds__(FR_BLOCK) k_fr_rows_apply(uint64_t* __restrict__ v, size_t n, const uint64_t* __restrict__ tsum,
                                                            unsigned long long* __restrict__ totals) {
    uint64_t* __restrict__ row = v + (size_t)blockIdx.y * n;
    const size_t t0 = (size_t)blockIdx.x * FR_TILE + (size_t)threadIdx.x * FR_ITEMS;
    uint64_t x[FR_ITEMS], sum = 0;
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        x[k] = t0 + k < n ? row[t0 + k] : 0ull;
        sum += x[k];
    }
    uint64_t total;
    uint64_t run = tsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive<FR_BLOCK>(sum, &total);
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        const size_t t = t0 + k;
        if (t >= n) break;
        row[t] = run;
        run += x[k];
        if (t == n - 1) totals[blockIdx.y] = run;
    }
}

// the tree that holds node 256 b of level l = blockIdx.y + 1: the largest t with C_l[t] <= 256 b
struct FirstRows {
    uint64_t off[FOREST_RAGGED_MAX_DEPTH + 1];
    uint64_t len[FOREST_RAGGED_MAX_DEPTH + 1];
};
__global__ void __launch_bounds__(FR_BLOCK) k_fr_block_first(const uint64_t* __restrict__ C, size_t n_trees, FirstRows fr,
                                                             uint64_t* __restrict__ first) {
    const unsigned l = blockIdx.y + 1;
    const size_t b = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (b >= fr.len[l]) return;
    const uint64_t* Crow = C + (size_t)l * (n_trees + 1);
    const uint64_t g = (uint64_t)b * 256;
    first[fr.off[l] + b] = last_at_or_below(Crow, 0, n_trees - 1, g);  // (C[0] = 0 <= g)
}

// ---- the digests of one level ----
struct FrLevel {
    const uint64_t* C;      // this level's node starts, n_trees + 1
    const uint64_t* Cprev;  // level l-1's (level-major scratch, l >= 2)
    const uint64_t* first;  // first tree of each 256-node block
    const uint64_t* LO;     // tree-major levels: each tree's block
    const uint64_t* ntree;
    const uint64_t* offsets;
    const Scalar32* leaves;
    const Scalar32* src;    // level-major scratch: level l-1
    Scalar32* dst;          // level-major scratch: level l
    Scalar32* levels;       // the caller's d_levels (tree-major), or null
    Scalar32* roots;
    size_t n_trees;
    size_t lanes;
    unsigned level, la;
};

// node g's tree and position, its children's array and its output slot.  false: no such node (g at or past the level's total).
struct FrNode {
    const Scalar32* children;
    uint64_t i, n_children;
    Scalar32* out;
};
__device__ __forceinline__ bool fr_node(const FrLevel& P, uint64_t g, FrNode& nd) {
    const uint64_t* __restrict__ C = P.C;
    if (g >= C[P.n_trees]) return false;
    const size_t t = last_at_or_below(C, P.first[g >> 8], P.first[(g >> 8) + 1], g);
    const uint64_t n = P.ntree[t];
    const unsigned l = P.level;
    nd.i = g - C[t];
    nd.n_children = ceil_shift(n, (l - 1) * P.la);
    if (P.levels) {
        Scalar32* blk = P.levels + P.LO[t];
        nd.children = l == 1 ? P.leaves + P.offsets[t] : blk + level_start(n, l - 1, P.la);
        nd.out = blk + level_start(n, l, P.la) + nd.i;
    } else {  // (a root is read by no later level: it goes to d_roots only)
        nd.children = l == 1 ? P.leaves + P.offsets[t] : P.src + P.Cprev[t];
        nd.out = ceil_shift(n, l * P.la) == 1 ? P.roots + t : P.dst + g;
    }
    return true;
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_fr_digest(const int32_t* __restrict__ tab, TagArg tag, FrLevel P) {
    const uint64_t g = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (g >= P.lanes) return;
    FrNode nd;
    if (!fr_node(P, g, nd)) return;
    E29 s[WIDTH];  // (written out, as in k_fu_digest: see the head of this file)
#pragma unroll
    for (int k = 0; k < NL; ++k) s[0].d[k] = tag.x0[k];  // lane 0 enters after its first S-box (hades_permute PRE0)
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const uint64_t c = nd.i * ARITY + k;
        if (k < ARITY && c < nd.n_children)
            s[1 + k] = load_scalar(nd.children + c);
        else
            s[1 + k] = e29_zero();
    }
    hades_permute<0x02u, true>(s, tab);  // only lane 1 is squeezed
    store_scalar(nd.out, s[1]);
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) k_fr_digest_coop(const int32_t* __restrict__ tab, TagArg tag, FrLevel P) {
    const uint64_t lane = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (lane >= P.lanes) return;  // (lanes is a multiple of 8: whole groups only)
    FrNode nd;
    if (!fr_node(P, lane >> 3, nd)) return;  // (the whole group: one node)
    const int j = (int)(threadIdx.x & 7u);
    const E29 digest = node_digest_coop<ARITY>(tab, tag, nd.children, nd.i, nd.n_children, j);
    if (j == 1) store_scalar(nd.out, digest);  // the digest is element 1 of the permuted state: lane 1's
}

// tree-major levels: each tree's root is the last scalar of its block (trees of one leaf and bad trees have theirs already)
__global__ void __launch_bounds__(FR_BLOCK) k_fr_roots_from_levels(const uint64_t* __restrict__ ntree, const uint64_t* __restrict__ LO,
                                                                   size_t n_trees, unsigned la, const Scalar32* __restrict__ levels,
                                                                   Scalar32* __restrict__ roots) {
    const size_t t = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (t >= n_trees) return;
    const uint64_t n = ntree[t];
    if (n < 2) return;
    const uint4* src = reinterpret_cast<const uint4*>(levels + LO[t] + levels_len_dev(n, la) - 1);
    uint4* dst = reinterpret_cast<uint4*>(roots + t);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---------------------------------------------------------------------------------------------
// the select: trees of one or two BUILT forests gathered into a new compact forest (p252_merkle{4,2}_forest_ragged_select_device_into).
// A tree's tree-major block holds what its own leaves give and nothing else, so nothing is hashed: leaves, level blocks and roots move.
//   k_fr_sel_sizes       per pick j: the leaf count s_j of the tree it names in A or B (0: an id out of range, a bad tree)
//   (k_fr_tile_sums / k_fr_scan_tiles / k_fr_scan_apply<true> over s_j with n_leaves = leaves_cap: the build's sum rule IS the cap
//    rule — a pick whose running sum passes leaves_cap is refused, and so is every later non-empty one)
//   k_fr_sel_offsets     the scan of the accepted counts: d_offsets_new
//   (launch_forest_ragged_index on d_offsets_new: the new forest's leaf counts and block starts are the build's own)
//   k_fr_sel_tile_first  per 512-scalar tile of the new leaves / of the new levels: the tree that holds its first scalar
//   k_fr_sel_move        one lane per 16-byte half of four scalars of the new array (leaves, then levels): its tree between the first
//                        trees of its tile and of the next, then the same place of the picked tree's block in its source
//   k_fr_sel_roots       the picked trees' roots; zero, and one count in *n_bad, for a refused pick
// ---------------------------------------------------------------------------------------------
namespace {
constexpr unsigned FRS_MOVE = 2 * FOREST_SELECT_MOVE_TILE / FR_BLOCK;  // 16-byte halves per lane of a relocation block

// the picked trees' starts (of their leaves, or of their level blocks) and the array they index, in either source
struct FrSelSrc {
    const uint64_t* start_a;
    const uint64_t* start_b;
    const uint4* data_a;
    const uint4* data_b;
    uint64_t n_trees_a;
};
}  // namespace

__global__ void __launch_bounds__(FR_BLOCK) k_fr_sel_sizes(const uint64_t* __restrict__ pick, size_t n_pick, const uint64_t* __restrict__ ntree_a,
                                                           uint64_t n_trees_a, const uint64_t* __restrict__ ntree_b, uint64_t n_trees_b,
                                                           uint64_t* __restrict__ count) {
    const size_t j = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (j >= n_pick) return;
    const uint64_t id = pick[j];
    uint64_t n = 0;
    if (id < n_trees_a)
        n = ntree_a[id];
    else if (id - n_trees_a < n_trees_b)
        n = ntree_b[id - n_trees_a];
    count[j] = n;
}

// out[j] = the accepted counts before pick j, out[n_pick] = their total (tsum: the tile sums of `count`, scanned)
__global__ void __launch_bounds__(FR_BLOCK) k_fr_sel_offsets(const uint64_t* __restrict__ count, size_t n_pick, const uint64_t* __restrict__ tsum,
                                                             uint64_t* __restrict__ out) {
    const size_t t0 = (size_t)blockIdx.x * FR_TILE + (size_t)threadIdx.x * FR_ITEMS;
    uint64_t v[FR_ITEMS], sum = 0;
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        v[k] = t0 + k < n_pick ? count[t0 + k] : 0ull;
        sum += v[k];
    }
    uint64_t total;
    uint64_t run = tsum[blockIdx.x] + block_exclusive<FR_BLOCK>(sum, &total);
#pragma unroll
    for (unsigned k = 0; k < FR_ITEMS; ++k) {
        const size_t t = t0 + k;
        if (t >= n_pick) break;
        out[t] = run;
        run += v[k];
        if (t == n_pick - 1) out[n_pick] = run;
    }
}

// the tree that holds scalar FOREST_SELECT_MOVE_TILE * b of B (n_trees + 1 starts): the largest t < n_trees with B[t] <= it
__global__ void __launch_bounds__(FR_BLOCK) k_fr_sel_tile_first(const uint64_t* __restrict__ B, size_t n_trees, size_t entries,
                                                                uint64_t* __restrict__ first) {
    const size_t b = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (b >= entries) return;
    first[b] = last_at_or_below(B, 0, n_trees - 1, (uint64_t)b * FOREST_SELECT_MOVE_TILE);  // (B[0] = 0)
}

// scalar s of the new array lies in new tree t (a pick that was accepted: only those have scalars), at s - B[t] of its block
__global__ void __launch_bounds__(FR_BLOCK) k_fr_sel_move(const uint64_t* __restrict__ B, size_t n_pick, const uint64_t* __restrict__ first,
                                                          const uint64_t* __restrict__ pick, FrSelSrc S, uint4* __restrict__ out) {
    const uint64_t total = B[n_pick];
    const size_t lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
#pragma unroll
    for (unsigned u = 0; u < FRS_MOVE; ++u) {
        const uint64_t h = ((uint64_t)blockIdx.x * FRS_MOVE + u) * FR_BLOCK + threadIdx.x;  // the 16-byte half
        const uint64_t s = h >> 1;
        if (s >= total) return;
        const size_t t = last_at_or_below(B, lo, hi, s);
        const uint64_t id = pick[t];
        const bool from_b = id >= S.n_trees_a;
        const uint64_t from = (from_b ? S.start_b[id - S.n_trees_a] : S.start_a[id]) + (s - B[t]);
        out[h] = (from_b ? S.data_b : S.data_a)[2 * from + (h & 1)];
    }
}

__global__ void __launch_bounds__(FR_BLOCK) k_fr_sel_roots(const uint64_t* __restrict__ ntree_new, size_t n_pick, const uint64_t* __restrict__ pick,
                                                           uint64_t n_trees_a, const uint4* __restrict__ roots_a, const uint4* __restrict__ roots_b,
                                                           Scalar32* __restrict__ roots, unsigned* __restrict__ n_bad) {
    const size_t j = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
    if (j >= n_pick) return;
    if (ntree_new[j] == 0) {  // refused: a good tree has a leaf
        store_zero(roots + j);
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    const uint64_t id = pick[j];
    const uint4* src = id >= n_trees_a ? roots_b + 2 * (id - n_trees_a) : roots_a + 2 * id;
    uint4* dst = reinterpret_cast<uint4*>(roots + j);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
unsigned forest_ragged_depth(size_t n, unsigned arity) {
    unsigned d = 0;
    for (size_t c = n; c > 1; c = c / arity + (c % arity != 0)) ++d;
    return d;
}

ForestRaggedPlan forest_ragged_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, bool levels) {
    ForestRaggedPlan p;
    p.arity = arity;
    p.log2a = arity == 4 ? 2 : 1;
    p.levels = levels;
    p.n_trees = n_trees;
    p.n_leaves = n_leaves;
    // a good tree has at most min(max_leaves, n_leaves) leaves
    p.depth = forest_ragged_depth(max_leaves < n_leaves ? max_leaves : n_leaves, arity);
    p.tiles = (n_trees + FR_TILE - 1) / FR_TILE;
    size_t words = n_trees + (size_t)(p.depth + 1) * (n_trees + 1) + (size_t)(p.depth + 1) * p.tiles;
    for (unsigned l = 1; l <= p.depth; ++l) {
        p.bound[l] = (n_leaves >> (l * p.log2a)) + n_trees;
        p.first_off[l] = words;
        p.first_len[l] = (p.bound[l] >> 8) + 2;
        words += p.first_len[l];
    }
    p.meta_bytes = (words * 8 + 255) & ~(size_t)255;
    return p;
}

// how the build and the index both start: k_fr_prep, then the scan of the leaf counts (with `roots`: those of bad and one-leaf trees)
static void launch_leaf_counts(const uint64_t* off, size_t n, size_t n_leaves, size_t max_leaves, size_t tiles, unsigned la, uint64_t* ntree,
                               uint64_t* tsum, uint64_t* C, const Scalar32* leaves, Scalar32* roots, unsigned* n_bad, hipStream_t st) {
    const dim3 blk(FR_BLOCK), grid((unsigned)tiles, 1);
    hipLaunchKernelGGL(k_fr_prep, dim3(grid_for(n)), blk, 0, st, off, n, (uint64_t)n_leaves, (uint64_t)max_leaves, ntree, leaves, roots);
    hipLaunchKernelGGL(k_fr_tile_sums, grid, blk, 0, st, ntree, n, FR_ROW_LEAVES, la, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3(1), blk, 0, st, tsum, tiles);
    hipLaunchKernelGGL(k_fr_scan_apply<true>, grid, blk, 0, st, ntree, n, FR_ROW_LEAVES, la, tsum, C, (uint64_t)n_leaves, off, leaves, roots, n_bad);
}

// the forest's index alone, for callers that read a built forest (forest_openings.hip): the validation and the leaf-count scan of
// the build (no roots written, nothing counted), then LO = the scan of levels_len(n_t)
size_t forest_ragged_index_bytes(size_t n_trees) {
    const size_t tiles = (n_trees + FR_TILE - 1) / FR_TILE;
    return ((2 * n_trees + 1 + tiles) * 8 + 255) & ~(size_t)255;
}

hipError_t launch_forest_ragged_index(unsigned arity, const void* offsets, size_t n_trees, size_t n_leaves, size_t max_leaves, void* meta,
                                      const uint64_t** ntree_out, const uint64_t** lo_out, hipStream_t st) {
    const size_t n = n_trees;
    const unsigned tiles = (unsigned)((n + FR_TILE - 1) / FR_TILE), la = arity == 4 ? 2 : 1;
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    uint64_t* ntree = static_cast<uint64_t*>(meta);
    uint64_t* LO = ntree + n;  // row 0 of C: n + 1 entries
    uint64_t* tsum = LO + n + 1;
    const dim3 blk(FR_BLOCK);
    *ntree_out = ntree;
    *lo_out = LO;
    if (n == 0) return hipSuccess;
    launch_leaf_counts(off, n, n_leaves, max_leaves, tiles, la, ntree, tsum, LO, nullptr, nullptr, nullptr, st);  // (no roots, nothing counted)
    hipLaunchKernelGGL(k_fr_tile_sums, dim3(tiles, 1), blk, 0, st, ntree, n, 0u, la, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3(1), blk, 0, st, tsum, (size_t)tiles);
    hipLaunchKernelGGL(k_fr_scan_apply<false>, dim3(tiles, 1), blk, 0, st, ntree, n, 0u, la, tsum, LO, (uint64_t)n_leaves, off,
                       (const Scalar32*)nullptr, (Scalar32*)nullptr, (unsigned*)nullptr);
    return hipGetLastError();
}

size_t forest_scan_rows_tiles(size_t n) { return (n + FR_TILE - 1) / FR_TILE; }

hipError_t launch_forest_scan_rows(uint64_t* values, size_t rows, size_t n, unsigned long long* totals, uint64_t* tsum, hipStream_t st) {
    if (rows == 0 || n == 0) return hipSuccess;
    const size_t tiles = forest_scan_rows_tiles(n);
    const dim3 blk(FR_BLOCK), grid((unsigned)tiles, (unsigned)rows);
    hipLaunchKernelGGL(k_fr_rows_tile_sums, grid, blk, 0, st, values, n, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3((unsigned)rows), blk, 0, st, tsum, tiles);
    hipLaunchKernelGGL(k_fr_rows_apply, grid, blk, 0, st, values, n, tsum, totals);
    return hipGetLastError();
}

hipError_t launch_forest_ragged(const int32_t* tab, const TagArg& tag, const ForestRaggedPlan& p, const void* leaves,
                                const void* offsets, size_t max_leaves, void* roots, void* levels, void* n_bad, void* meta,
                                void* lvl_a, void* lvl_b, hipStream_t st) {
    const size_t n = p.n_trees;
    if (n == 0) return hipSuccess;
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    const Scalar32* lv = static_cast<const Scalar32*>(leaves);
    Scalar32* rt = static_cast<Scalar32*>(roots);
    unsigned* nb = static_cast<unsigned*>(n_bad);
    uint64_t* ntree = static_cast<uint64_t*>(meta);
    uint64_t* C = ntree + n;
    uint64_t* tsum = C + (size_t)(p.depth + 1) * (n + 1);
    uint64_t* first = static_cast<uint64_t*>(meta);
    const unsigned la = p.log2a;
    const dim3 blk(FR_BLOCK);
    launch_leaf_counts(off, n, p.n_leaves, max_leaves, p.tiles, la, ntree, tsum, C, lv, rt, nb, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.depth == 0) return e;
    // every level's node starts (and LO, the tree-major levels' block starts, in row 0)
    const unsigned row0 = p.levels ? 0u : 1u, rows = p.depth + 1 - row0;
    hipLaunchKernelGGL(k_fr_tile_sums, dim3((unsigned)p.tiles, rows), blk, 0, st, ntree, n, row0, la, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3(rows), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fr_scan_apply<false>, dim3((unsigned)p.tiles, rows), blk, 0, st, ntree, n, row0, la, tsum, C,
                       (uint64_t)p.n_leaves, off, lv, rt, nb);
    FirstRows fr = {};
    for (unsigned l = 1; l <= p.depth; ++l) {
        fr.off[l] = p.first_off[l];
        fr.len[l] = p.first_len[l];
    }
    hipLaunchKernelGGL(k_fr_block_first, dim3(grid_for(p.first_len[1]), p.depth), blk, 0, st, C, n, fr, first);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (unsigned l = 1; l <= p.depth; ++l) {
        FrLevel P;
        P.C = C + (size_t)l * (n + 1);
        P.Cprev = C + (size_t)(l - 1) * (n + 1);
        P.first = first + p.first_off[l];
        P.LO = C;
        P.ntree = ntree;
        P.offsets = off;
        P.leaves = lv;
        P.src = static_cast<const Scalar32*>((l & 1) ? lvl_b : lvl_a);  // level l-1 (odd levels live in lvl_a)
        P.dst = static_cast<Scalar32*>((l & 1) ? lvl_a : lvl_b);
        P.levels = static_cast<Scalar32*>(levels);
        P.roots = rt;
        P.n_trees = n;
        P.level = l;
        P.la = la;
        const bool coop = coop8(p.bound[l]);
        P.lanes = coop ? p.bound[l] * 8 : p.bound[l];
        if (p.arity == 4)
            e = launch(coop ? k_fr_digest_coop<4> : k_fr_digest<4>, P.lanes, st, tab, tag, P);
        else
            e = launch(coop ? k_fr_digest_coop<2> : k_fr_digest<2>, P.lanes, st, tab, tag, P);
        if (e != hipSuccess) return e;
    }
    if (p.levels)
        hipLaunchKernelGGL(k_fr_roots_from_levels, dim3(grid_for(n)), blk, 0, st, ntree, C, n, la, static_cast<const Scalar32*>(levels), rt);
    return hipGetLastError();
}

ForestSelectPlan forest_select_plan(unsigned arity, size_t n_trees_a, size_t n_trees_b, size_t max_leaves, size_t n_pick, size_t leaves_cap) {
    ForestSelectPlan p;
    p.arity = arity;
    p.depth = forest_ragged_depth(max_leaves, arity);
    p.n_pick = n_pick;
    p.leaves_cap = leaves_cap;
    p.max_leaves = max_leaves;
    p.nodes = leaves_cap / (arity - 1) + n_pick * p.depth;
    p.tiles = (n_pick + FR_TILE - 1) / FR_TILE;
    p.leaf_tiles = (leaves_cap + FOREST_SELECT_MOVE_TILE - 1) / FOREST_SELECT_MOVE_TILE;
    p.node_tiles = (p.nodes + FOREST_SELECT_MOVE_TILE - 1) / FOREST_SELECT_MOVE_TILE;
    p.index_a_bytes = forest_ragged_index_bytes(n_trees_a);
    p.index_b_bytes = forest_ragged_index_bytes(n_trees_b);
    p.index_new_bytes = forest_ragged_index_bytes(n_pick);
    // one count per pick, the scans' tile sums, the two first-tree rows
    const size_t words = n_pick + p.tiles + p.leaf_tiles + 1 + p.node_tiles + 1;
    p.work_bytes = (words * 8 + 255) & ~(size_t)255;
    return p;
}

hipError_t launch_forest_select(const ForestSelectPlan& p, const ForestSelectSource& A, const ForestSelectSource& B, const void* pick,
                                void* leaves_new, void* offsets_new, void* levels_new, void* roots_new, void* n_bad, void* meta,
                                hipStream_t st) {
    const size_t n = p.n_pick;
    if (n == 0) return hipSuccess;
    char* base = static_cast<char*>(meta);
    const uint64_t *ntree_a = nullptr, *lo_a = nullptr, *ntree_b = nullptr, *lo_b = nullptr, *ntree_new = nullptr, *lo_new = nullptr;
    hipError_t e = launch_forest_ragged_index(p.arity, A.offsets, A.n_trees, A.n_leaves, A.max_leaves, base, &ntree_a, &lo_a, st);
    if (e != hipSuccess) return e;
    e = launch_forest_ragged_index(p.arity, B.offsets, B.n_trees, B.n_leaves, B.max_leaves, base + p.index_a_bytes, &ntree_b, &lo_b, st);
    if (e != hipSuccess) return e;
    uint64_t* count = reinterpret_cast<uint64_t*>(base + p.index_a_bytes + p.index_b_bytes + p.index_new_bytes);
    uint64_t* tsum = count + n;
    uint64_t* first_leaf = tsum + p.tiles;
    uint64_t* first_node = first_leaf + p.leaf_tiles + 1;
    const uint64_t* pk = static_cast<const uint64_t*>(pick);
    uint64_t* off_new = static_cast<uint64_t*>(offsets_new);
    const unsigned la = p.arity == 4 ? 2 : 1;
    const dim3 blk(FR_BLOCK), per_pick(grid_for(n)), tiles((unsigned)p.tiles, 1);

    hipLaunchKernelGGL(k_fr_sel_sizes, per_pick, blk, 0, st, pk, n, ntree_a, (uint64_t)A.n_trees, ntree_b, (uint64_t)B.n_trees, count);
    // the cap rule: the build's sum rule over the picks' counts, with leaves_cap for n_leaves (no roots, nothing counted)
    hipLaunchKernelGGL(k_fr_tile_sums, tiles, blk, 0, st, count, n, FR_ROW_LEAVES, la, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3(1), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fr_scan_apply<true>, tiles, blk, 0, st, count, n, FR_ROW_LEAVES, la, tsum, (uint64_t*)nullptr, (uint64_t)p.leaves_cap,
                       (const uint64_t*)nullptr, (const Scalar32*)nullptr, (Scalar32*)nullptr, (unsigned*)nullptr);
    hipLaunchKernelGGL(k_fr_tile_sums, tiles, blk, 0, st, count, n, FR_ROW_LEAVES, la, tsum);
    hipLaunchKernelGGL(k_fr_scan_tiles, dim3(1), blk, 0, st, tsum, p.tiles);
    hipLaunchKernelGGL(k_fr_sel_offsets, tiles, blk, 0, st, count, n, tsum, off_new);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the new forest's index: the build's own validation and block starts, on the offsets just written
    e = launch_forest_ragged_index(p.arity, off_new, n, p.leaves_cap, p.max_leaves, base + p.index_a_bytes + p.index_b_bytes, &ntree_new, &lo_new, st);
    if (e != hipSuccess) return e;

    FrSelSrc S;
    S.n_trees_a = A.n_trees;
    S.start_a = static_cast<const uint64_t*>(A.offsets);
    S.start_b = static_cast<const uint64_t*>(B.offsets);
    S.data_a = static_cast<const uint4*>(A.leaves);
    S.data_b = static_cast<const uint4*>(B.leaves);
    hipLaunchKernelGGL(k_fr_sel_tile_first, dim3(grid_for(p.leaf_tiles + 1)), blk, 0, st, off_new, n, p.leaf_tiles + 1, first_leaf);
    hipLaunchKernelGGL(k_fr_sel_move, dim3((unsigned)p.leaf_tiles), blk, 0, st, off_new, n, first_leaf, pk, S, static_cast<uint4*>(leaves_new));
    if (p.depth && p.nodes) {
        S.start_a = lo_a;
        S.start_b = lo_b;
        S.data_a = static_cast<const uint4*>(A.levels);
        S.data_b = static_cast<const uint4*>(B.levels);
        hipLaunchKernelGGL(k_fr_sel_tile_first, dim3(grid_for(p.node_tiles + 1)), blk, 0, st, lo_new, n, p.node_tiles + 1, first_node);
        hipLaunchKernelGGL(k_fr_sel_move, dim3((unsigned)p.node_tiles), blk, 0, st, lo_new, n, first_node, pk, S, static_cast<uint4*>(levels_new));
    }
    hipLaunchKernelGGL(k_fr_sel_roots, per_pick, blk, 0, st, ntree_new, n, pk, (uint64_t)A.n_trees, static_cast<const uint4*>(A.roots),
                       static_cast<const uint4*>(B.roots), static_cast<Scalar32*>(roots_new), static_cast<unsigned*>(n_bad));
    return hipGetLastError();
}

}  // namespace p252
