// forest_update.hip — k leaf updates (tree id, leaf id, new leaf) anywhere in a built forest of trees of DIFFERENT sizes
// (forest_ragged.hip, tree-major levels) in one call, for both arities, every dirty node hashed ONCE.  k_merkle4_update
// (kernels.hip) hashes k nodes on every level — at the root level all k lanes hash the same node; here each level's dirty nodes are
// first made distinct, then hashed:
//   k_fu_scatter   one lane per update: validated as k_fo_record validates an opening, through forest_tree_leaves (tree id <
//                  n_trees, a good tree, leaf id < n_t — one count in *n_bad otherwise, nothing written), the new leaf stored (two 16-byte stores), a 16-byte
//                  record (tree id, valid, leaf id) written as list 0; a single-leaf tree's root is its leaf, reduced
//   k_fu_claim     level l = 1 .. D, one lane per record of list l - 1: the parent (t, i >> log2 arity), keyed by its slot in d_levels
//                  (LO[t] + level_start(n_t, l) + i, unique across the forest), is claimed in an open-addressing table with one
//                  64-bit compare-and-swap (empty -> key, linear probing, at most half full).  The lane whose swap installs the
//                  key appends the parent to list l (one atomic add per wave: ballot, popcount, the leader's base broadcast);
//                  every other lane drops out, and so do the records of trees that ended below level l.
//   k_fu_digest / k_fu_digest_coop   lane (group of 8 lanes) g < count[l] hashes record g of list l: children a i .. a i + a - 1 of
//                  level l - 1 of the tree (its leaves for l = 1; zero at or past s_{l-1}(t)), output to level l of the tree's
//                  block, and to d_roots[t] when the node is the tree's only one at that level.  The launch has min(k, bound[l])
//                  lanes and leaves on the device-side count: the host never learns it.  Lane 0 adds the count to *n_hashed.
// A level's digest launch reads level l - 1 and writes level l only, so updating in place is race-free across launch boundaries.
// The permutation is the library's, as in k_fr_digest / k_fr_digest_coop: hades_permute<0x02u, true> with the hoisted tag S-box at
// 3 waves per SIMD (written out here as there: forest_ragged.hip says why), node_digest_coop when the level cannot fill the chip (the
// coop8 rule of kernels.h on min(k, bound[l])).  The closed forms, u64_of and the tree lookup are forest_node.hpp's too.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_node.hpp"
#include "forest_update.h"
#include "hades29.hpp"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FU_BLOCK = 256;

}  // namespace

// ---- the leaves, and list 0 ----
__global__ void __launch_bounds__(FU_BLOCK) k_fu_scatter(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                         size_t n_trees, const uint32_t* __restrict__ tree_ids,
                                                         const uint64_t* __restrict__ leaf_ids, const uint4* __restrict__ new_leaves,
                                                         size_t k, uint4* __restrict__ leaves, uint4* __restrict__ roots,
                                                         uint4* __restrict__ list, unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * FU_BLOCK + threadIdx.x;
    if (i >= k) return;
    const uint32_t t = tree_ids[i];
    const uint64_t leaf = leaf_ids[i];
    size_t ts;
    const uint64_t n = forest_tree_leaves(ntree, n_trees, t, &ts);
    if (n == 0 || leaf >= n) {  // a bad update: nothing written, no record
        list[i] = make_uint4(0u, 0u, 0u, 0u);
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    const uint4 lo = new_leaves[2 * i], hi = new_leaves[2 * i + 1];
    const size_t at = 2 * (size_t)(offsets[ts] + leaf);  // (inside the tree: k_fr_prep checked offsets[t + 1] <= n_leaves)
    leaves[at] = lo;
    leaves[at + 1] = hi;
    if (n == 1 && roots)  // (the leaf keeps its bytes; the root is reduced, as every output and as the forest's build writes it)
        store_scalar(reinterpret_cast<Scalar32*>(roots) + ts, load_scalar(reinterpret_cast<const Scalar32*>(new_leaves) + i));
    list[i] = record(t, leaf);
}

// ---- level l's distinct dirty nodes: list l - 1 -> list l ----
__global__ void __launch_bounds__(FU_BLOCK) k_fu_claim(const uint4* __restrict__ in, const unsigned long long* __restrict__ in_count,
                                                       size_t lanes, const uint64_t* __restrict__ ntree, const uint64_t* __restrict__ LO,
                                                       unsigned l, unsigned la, unsigned long long* __restrict__ table, unsigned shift,
                                                       uint4* __restrict__ out, unsigned long long* __restrict__ out_count) {
    const size_t g = (size_t)blockIdx.x * FU_BLOCK + threadIdx.x;
    // (no early return: the whole wave takes part in the append below)
    bool live = g < lanes && (!in_count || g < *in_count);
    const uint4 r = live ? in[g] : make_uint4(0u, 0u, 0u, 0u);
    live = live && r.y != 0;
    const uint32_t t = r.x;
    const uint64_t n = live ? ntree[t] : 0ull;
    live = live && ceil_shift(n, (l - 1) * la) > 1;  // level l - 1 has more than one node: the tree has a level l
    const uint64_t parent = u64_of(r.z, r.w) >> la;
    const bool won = live && claim(table, shift, LO[t] + level_start(n, l, la) + parent);
    const unsigned long long winners = __ballot(won);
    if (winners == 0) return;
    const unsigned long long place = append_place(won, winners, out_count);
    if (won) out[place] = record(t, parent);
}

// ---- the digests of one level ----
struct FuLevel {
    const uint4* list;                 // this level's records
    const unsigned long long* count;   // how many
    const uint64_t* ntree;
    const uint64_t* LO;
    const uint64_t* offsets;
    const Scalar32* leaves;
    Scalar32* levels;
    Scalar32* roots;                   // may be null
    unsigned long long* n_hashed;      // may be null
    size_t lanes;
    unsigned level, la;
};

struct FuNode {
    const Scalar32* children;
    uint64_t i, n_children;
    Scalar32* out;
    Scalar32* root;  // null unless the node is its tree's root and the caller wants the roots
};
__device__ __forceinline__ bool fu_node(const FuLevel& P, uint64_t g, FuNode& nd) {
    if (g >= *P.count) return false;
    const uint4 r = P.list[g];
    const size_t t = r.x;
    const uint64_t n = P.ntree[t];
    const unsigned l = P.level;
    nd.i = u64_of(r.z, r.w);
    nd.n_children = ceil_shift(n, (l - 1) * P.la);
    Scalar32* blk = P.levels + P.LO[t];
    const uint64_t below = level_start(n, l - 1, P.la);  // (level_start(n, 0) = level_start(n, 1) = 0)
    nd.children = l == 1 ? P.leaves + P.offsets[t] : blk + below;
    nd.out = blk + (l == 1 ? 0 : below + nd.n_children) + nd.i;
    nd.root = P.roots && ceil_shift(n, l * P.la) == 1 ? P.roots + t : nullptr;
    return true;
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_fu_digest(const int32_t* __restrict__ tab, TagArg tag, FuLevel P) {
    const uint64_t g = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (g >= P.lanes) return;
    if (g == 0 && P.n_hashed) atomicAdd(P.n_hashed, *P.count);
    FuNode nd;
    if (!fu_node(P, g, nd)) return;
    E29 s[WIDTH];  // (written out, as in k_fr_digest: see the head of this file)
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
    if (nd.root) store_scalar(nd.root, s[1]);
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) k_fu_digest_coop(const int32_t* __restrict__ tab, TagArg tag, FuLevel P) {
    const uint64_t lane = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (lane >= P.lanes) return;  // (lanes is a multiple of 8: whole groups only)
    if (lane == 0 && P.n_hashed) atomicAdd(P.n_hashed, *P.count);
    FuNode nd;
    if (!fu_node(P, lane >> 3, nd)) return;  // (the whole group: one node)
    const int j = (int)(threadIdx.x & 7u);
    const E29 mine = node_digest_coop<ARITY>(tab, tag, nd.children, nd.i, nd.n_children, j);
    if (j == 1) {  // the digest is element 1 of the permuted state: lane 1's
        store_scalar(nd.out, mine);
        if (nd.root) store_scalar(nd.root, mine);
    }
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
ForestUpdatePlan forest_update_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k) {
    const ForestRaggedPlan fr = forest_ragged_plan(arity, n_leaves, n_trees, max_leaves, true);
    ForestUpdatePlan p;
    p.arity = arity;
    p.log2a = fr.log2a;
    p.depth = fr.depth;
    p.n_trees = n_trees;
    p.k = k;
    p.in[0] = k;
    size_t widest = 0;
    for (unsigned l = 1; l <= p.depth; ++l) {
        p.in[l] = k < fr.bound[l] ? k : fr.bound[l];
        size_t slots = CLAIM_MIN_SLOTS;
        while (slots < 2 * p.in[l - 1]) slots <<= 1;
        p.slots[l] = slots;
        if (slots > widest) widest = slots;
    }
    p.list_bytes = k * sizeof(uint4);
    p.count_bytes = ((size_t)(p.depth + 1) * sizeof(unsigned long long) + 255) & ~(size_t)255;
    p.table_bytes = widest * sizeof(unsigned long long);
    return p;
}

// one level's digests over a list made by the caller (launch_forest_update below, forest_append.hip): the 8-lane kernel when the
// list's host bound cannot fill the chip (the coop8 rule of kernels.h)
hipError_t launch_forest_digest_list(const int32_t* tab, const TagArg& tag, unsigned arity, unsigned log2a, const ForestDigestList& d,
                                     hipStream_t st) {
    if (d.bound == 0) return hipSuccess;
    FuLevel P;
    P.list = static_cast<const uint4*>(d.list);
    P.count = d.count;
    P.ntree = d.ntree;
    P.LO = d.lo;
    P.offsets = static_cast<const uint64_t*>(d.offsets);
    P.leaves = static_cast<const Scalar32*>(d.leaves);
    P.levels = static_cast<Scalar32*>(d.levels);
    P.roots = static_cast<Scalar32*>(d.roots);
    P.n_hashed = static_cast<unsigned long long*>(d.n_hashed);
    P.level = d.level;
    P.la = log2a;
    const bool coop = coop8(d.bound);
    P.lanes = coop ? d.bound * 8 : d.bound;
    if (arity == 4) return launch(coop ? k_fu_digest_coop<4> : k_fu_digest<4>, P.lanes, st, tab, tag, P);
    return launch(coop ? k_fu_digest_coop<2> : k_fu_digest<2>, P.lanes, st, tab, tag, P);
}

hipError_t launch_forest_update(const int32_t* tab, const TagArg& tag, const ForestUpdatePlan& p, void* leaves, const void* offsets,
                                const uint64_t* ntree, const uint64_t* lo, void* levels, const void* tree_ids, const void* leaf_ids,
                                const void* new_leaves, void* roots, void* n_bad, void* n_hashed, void* ids, void* table, hipStream_t st) {
    if (p.k == 0) return hipSuccess;
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    hipLaunchKernelGGL(k_fu_scatter, dim3((unsigned)((p.k + FU_BLOCK - 1) / FU_BLOCK)), dim3(FU_BLOCK), 0, st, off, ntree, p.n_trees,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint64_t*>(leaf_ids), static_cast<const uint4*>(new_leaves),
                       p.k, static_cast<uint4*>(leaves), static_cast<uint4*>(roots), p.list(ids, 0), static_cast<unsigned*>(n_bad));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.depth == 0) return e;
    ForestDigestList d;
    d.ntree = ntree;
    d.lo = lo;
    d.offsets = offsets;
    d.leaves = leaves;
    d.levels = levels;
    d.roots = roots;
    d.n_hashed = n_hashed;
    return launch_forest_update_levels(tab, tag, p, d, ids, table, st, [&](const ForestClaimLevel& c) {
        hipLaunchKernelGGL(k_fu_claim, dim3((unsigned)((c.lanes + FU_BLOCK - 1) / FU_BLOCK)), dim3(FU_BLOCK), 0, st, c.in, c.in_count, c.lanes,
                           ntree, lo, c.level, p.log2a, c.table, c.shift, c.out, c.out_count);
    });
}

}  // namespace p252
