// forest_witness.hip — the openings of marked leaves kept current across an append to a forest kept only as its frontiers
// (p252_merkle{4,2}_forest_frontier_append_witness_device_into): one launch between the append's last digest launch and k_ff_finish
// (forest_frontier.hip), which hashes nothing.  With A = arity, f_l(n) = floor(n / A^l) and c_l(n) = ceil(n / A^l), an append from n to
// n' computes V_l = the nodes [f_l(n), c_l(n')) of every level l (V_0 = the new leaves), and the sibling x of any opening on level l is
// FINAL (x < f_l(n): in a witness that was current at n — or, for a leaf that this very append brings, in the frontier's OLD row l at
// slot x - A f_{l+1}(n): the path's node is at or past f_l(n), so its group is the partly filled one), in V_l (x < c_l(n')), or zero.
//   k_fw_refresh   one lane per (witness, row): the row's A - 1 siblings and its position byte; the lane of row 0 also writes the
//                  leaf, the depth byte and the bad count.  Witness i of tree t, leaf p, n = the tree's count before and n' after:
//                    t >= n_trees or p >= n'            bad: all zero, depth 0xFF, counted
//                    p < n, n' == n                     untouched (counted if its depth byte is 0xFF already)
//                    p < n, n' > n                      depth byte != depth(n) (0xFF included): bad.  Else rows l < depth(n'): a row
//                                                       whose group is final (p / A^(l+1) < f_{l+1}(n)) stays, in any other the
//                                                       final siblings stay and the rest come from V_l or are zero; rows at or past
//                                                       depth(n') stay (zero in an opening at n); the leaf stays
//                    n <= p < n'                        the input is ignored: every row l < depth(n') from the old frontier row, V_l
//                                                       and zero, the rows above zero, the leaf from d_add
// The layout is p252_merkle{4,2}_forest_ragged_openings_device's (forest_openings.hip, k_fr_openings): row l holds its group's nodes in
// index order with the path's own node left out.  The depth byte is read by every lane of its witness and written by one of them:
// a block holds floor(256 / D) WHOLE witnesses and a barrier stands between its reads and its stores, so the lanes of a block are the
// rows [blockIdx.x * per_block * D ..) in order and a wave's stores are one contiguous run, (A - 1) * 32 bytes per lane.
#include <hip/hip_runtime.h>

#include "forest_node.hpp"
#include "forest_witness.h"

namespace p252 {

namespace {

constexpr unsigned FW_BLOCK = FOREST_WITNESS_BLOCK;
constexpr unsigned FW_BAD_DEPTH = 0xFF;  // FOREST_OPENINGS_BAD_DEPTH (forest_openings.h)

__device__ __forceinline__ uint64_t floor_shift(uint64_t n, unsigned k) { return k >= 64 ? 0ull : n >> k; }

__device__ __forceinline__ void copy_scalar(uint4* __restrict__ dst, const uint4* __restrict__ src) {
    dst[0] = src[0];
    dst[1] = src[1];
}

__device__ __forceinline__ void zero_scalar(uint4* __restrict__ dst) {
    dst[0] = make_uint4(0u, 0u, 0u, 0u);
    dst[1] = make_uint4(0u, 0u, 0u, 0u);
}

// p252_merkle{4,2}_depth(n)
__device__ __forceinline__ unsigned depth_of(uint64_t n, unsigned la) {
    unsigned d = 0;
#pragma unroll 1
    for (uint64_t c = n; c > 1; c = ceil_shift(c, la)) ++d;
    return d;
}

}  // namespace

template <unsigned ARITY>
__global__ void __launch_bounds__(FW_BLOCK) k_fw_refresh(ForestFrontierView V, ForestWitnesses W, unsigned D, unsigned per_block) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1, PER = ARITY - 1;
    const unsigned w = D ? threadIdx.x / D : threadIdx.x;  // the witness inside the block, and its row
    const unsigned l = D ? threadIdx.x - w * D : 0u;
    const size_t i = (size_t)blockIdx.x * per_block + w;
    const bool live = w < per_block && i < W.k;
    size_t t = 0;
    uint64_t p = 0, n = 0, m = 0;
    unsigned din = 0;
    if (live) {
        t = W.tree_ids[i];
        p = W.leaf_ids[i];
        din = W.depths[i];
        if (t < V.n_trees) {  // (an unknown tree: n' = 0, so the witness is bad)
            n = V.nold[t];
            m = V.madd[t];
        }
    }
    __syncthreads();  // every lane of a witness has read its depth byte before the lane of row 0 stores it
    if (!live) return;
    const uint64_t nn = n + m;  // (m <= max_leaves - n: k_ff_sizes)
    const bool carried = p < n, first = l == 0;
    if (carried && m == 0) {  // an unchanged tree: byte for byte as it was
        if (first && din == FW_BAD_DEPTH && W.n_bad) atomicAdd(W.n_bad, 1u);
        return;
    }
    const bool bad = p >= nn || (carried && din != depth_of(n, LA));
    const unsigned top = bad ? 0u : depth_of(nn, LA);  // depth(n') >= 1 from here on unless D == 0: the tree grew past one leaf
    if (D) {
        uint4* row = static_cast<uint4*>(W.siblings) + 2 * PER * (i * D + l);
        uint8_t* pos = W.positions + (i * D + l);
        if (bad || l >= top) {
            if (bad || !carried) {
#pragma unroll
                for (unsigned j = 0; j < PER; ++j) zero_scalar(row + 2 * j);
                *pos = 0;
            }
        } else {
            const uint64_t node = p >> (l * LA);  // (l < D <= 64 / LA)
            const unsigned slot = (unsigned)(node & (ARITY - 1));
            const uint64_t f = n >> (l * LA), up = floor_shift(n, (l + 1) * LA), c = ceil_shift(nn, l * LA);
            if (!(carried && floor_shift(p, (l + 1) * LA) < up)) {  // (a carried row whose whole group is final stays)
                // V_l of this tree, and the old row l of its frontier
                const uint4* run = l == 0 ? static_cast<const uint4*>(V.add) + 2 * V.add_offsets[t]
                                          : static_cast<const uint4*>(V.values) + 2 * (V.list_off[l] + V.rows[(size_t)l * (V.n_trees + 1) + t]);
                const uint4* old = static_cast<const uint4*>(V.frontier) + 2 * ((uint64_t)t * V.stride + (uint64_t)l * PER);
#pragma unroll
                for (unsigned j = 0; j < PER; ++j) {
                    const uint64_t x = node - slot + j + (j >= slot ? 1u : 0u);  // the group's nodes in order, the path's own left out
                    if (x < f) {
                        if (!carried) copy_scalar(row + 2 * j, old + 2 * (x - (up << LA)));  // (x >= A f_{l+1}(n): see above)
                    } else if (x < c) {
                        copy_scalar(row + 2 * j, run + 2 * (x - f));
                    } else {
                        zero_scalar(row + 2 * j);
                    }
                }
                *pos = (uint8_t)slot;
            }
        }
    }
    if (!first) return;
    uint4* leaf = static_cast<uint4*>(W.leaves) + 2 * i;
    if (bad)
        zero_scalar(leaf);
    else if (!carried)
        copy_scalar(leaf, static_cast<const uint4*>(V.add) + 2 * (V.add_offsets[t] + (p - n)));
    W.depths[i] = bad ? (uint8_t)FW_BAD_DEPTH : (uint8_t)top;
    if (bad && W.n_bad) atomicAdd(W.n_bad, 1u);
}

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from forest_frontier.hip)
// ---------------------------------------------------------------------------------------------
hipError_t launch_forest_witness_refresh(const ForestFrontierView& view, const ForestWitnesses& witnesses, hipStream_t st) {
    if (witnesses.k == 0) return hipSuccess;
    const unsigned D = view.depth, per_block = D ? FW_BLOCK / D : FW_BLOCK;  // (D <= FOREST_RAGGED_MAX_DEPTH = 64)
    const dim3 grid((unsigned)forest_witness_blocks(witnesses.k, D)), blk(FW_BLOCK);
    if (view.log2a == 2)
        hipLaunchKernelGGL(k_fw_refresh<4>, grid, blk, 0, st, view, witnesses, D, per_block);
    else
        hipLaunchKernelGGL(k_fw_refresh<2>, grid, blk, 0, st, view, witnesses, D, per_block);
    return hipGetLastError();
}

}  // namespace p252
