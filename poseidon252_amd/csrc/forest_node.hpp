// forest_node.hpp — device code shared by the kernels of the ragged forest (forest_ragged.hip, forest_openings.hip, forest_update.hip):
// the closed forms of one tree's levels inside its tree-major block, the lookup of a tree in the forest's index, and the 8-lane digest
// of one node.  The permutation is the library's (hades29.hpp, coop29.hpp), included here and never copied.
#pragma once
#include "coop29.hpp"
#include "hades29.hpp"
#include "kernels.h"

namespace p252 {

// ---- the closed forms of one tree's levels (tree-major: levels 1, 2, .. of a tree one after the other in its block) ----
// ceil(n / 2^k) for any k
__device__ __forceinline__ uint64_t ceil_shift(uint64_t n, unsigned k) {
    if (k >= 64) return n != 0;
    return (n >> k) + ((n & ((1ull << k) - 1)) != 0);
}
// nodes of level l >= 1 of a tree of n leaves (0: the tree ended below l)
__device__ __forceinline__ uint64_t level_nodes(uint64_t n, unsigned l, unsigned la) {
    return ceil_shift(n, (l - 1) * la) > 1 ? ceil_shift(n, l * la) : 0;
}
// p252_merkle{4,2}_levels_len(n)
__device__ __forceinline__ uint64_t levels_len_dev(uint64_t n, unsigned la) {
    uint64_t total = 0;
#pragma unroll 1
    for (uint64_t c = n; c > 1;) {
        c = ceil_shift(c, la);
        total += c;
    }
    return total;
}
// start of level l >= 1 inside the levels block of a tree of n leaves (levels 1 .. l-1 before it)
__device__ __forceinline__ uint64_t level_start(uint64_t n, unsigned l, unsigned la) {
    uint64_t w = 0;
#pragma unroll 1
    for (unsigned j = 1; j < l; ++j) w += ceil_shift(n, j * la);
    return w;
}
__device__ __forceinline__ uint64_t u64_of(unsigned lo, unsigned hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
// the eight words of a stored scalar, reduced: V < 2^256 < 3 p, so two conditional subtractions (what store_scalar(load_scalar())
// gives, without the change of radix) — the forest's convention for a one-leaf tree: its root is its leaf mod p
__device__ __forceinline__ void words_mod_p(uint4& lo, uint4& hi) {
    const uint64_t P0 = 0xffffffff00000001ull, P1 = 0x53bda402fffe5bfeull, P2 = 0x3339d80809a1d805ull, P3 = 0x73eda753299d7d48ull;
    uint64_t v0 = u64_of(lo.x, lo.y), v1 = u64_of(lo.z, lo.w), v2 = u64_of(hi.x, hi.y), v3 = u64_of(hi.z, hi.w);
#pragma unroll 1
    for (int rep = 0; rep < 2; ++rep) {
        const bool ge = v3 != P3 ? v3 > P3 : v2 != P2 ? v2 > P2 : v1 != P1 ? v1 > P1 : v0 >= P0;
        if (ge) {  // V -= p, limb by limb with the borrow
            const uint64_t b0 = v0 < P0, t1 = v1 - P1, t2 = v2 - P2;
            const uint64_t b1 = (v1 < P1) | (t1 < b0);
            v0 -= P0;
            v1 = t1 - b0;
            const uint64_t b2 = (v2 < P2) | (t2 < b1);
            v2 = t2 - b1;
            v3 = v3 - P3 - b2;
        }
    }
    lo = make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
    hi = make_uint4((unsigned)v2, (unsigned)(v2 >> 32), (unsigned)v3, (unsigned)(v3 >> 32));
}
// a record of the level lists (16 bytes: tree id, valid, node index low and high), as k_fu_claim writes it and k_fu_digest reads it
// (forest_update.h); a void record is all zero
__device__ __forceinline__ uint4 record(uint32_t t, uint64_t i) { return make_uint4(t, 1u, (unsigned)i, (unsigned)(i >> 32)); }

// ---- a tree id of a (tree id, leaf id) pair against the forest's index (launch_forest_ragged_index): n_t, or 0 for an unknown
// (t >= n_trees) or a bad tree.  *ts = t, or 0 for an unknown tree: safe for the per-tree arrays (n_trees >= 1: entry 0 exists) ----
__device__ __forceinline__ uint64_t forest_tree_leaves(const uint64_t* __restrict__ ntree, size_t n_trees, size_t t, size_t* ts) {
    const bool known = t < n_trees;
    *ts = known ? t : 0;
    return known ? ntree[*ts] : 0ull;
}

// ---- the digest of node i of a level by a group of 8 lanes: children[ARITY i .. ARITY i + ARITY - 1] of the level below, zero at
// or past n_children.  j = the lane's place in its group; every lane of the group calls this, and the digest is element 1 of the
// permuted state: the value returned to lane j == 1.  (The one-lane form, hades_permute<0x02u, true> over the same children, is
// written out in k_fr_digest and k_fu_digest: forest_ragged.hip says why.) ----
template <unsigned ARITY>
__device__ __forceinline__ E29 node_digest_coop(const int32_t* __restrict__ tab, const TagArg& tag, const Scalar32* children, uint64_t i,
                                                uint64_t n_children, int j) {
    const int el = j < WIDTH ? j : WIDTH - 1;  // the state element this lane brings: 0 = tag, 1..4 = children
    E29 mine = from_mont4(tag.w);
    if (el > 0) {
        const uint64_t c = i * ARITY + (uint64_t)(el - 1);
        mine = (unsigned)(el - 1) < ARITY && c < n_children ? load_scalar(children + c) : e29_zero();
    }
    E29 last = mine;
    WaveComm8 cm{j, (int)(((threadIdx.x & 63u) & ~7u) * 4u)};
    CoopLane<8> L = coop_lane<8>(tab, cm);
    hades_permute_coop<8, false>(mine, last, tab, cm, L);
    return mine;
}

}  // namespace p252
