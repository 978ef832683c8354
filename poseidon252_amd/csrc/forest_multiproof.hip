// forest_multiproof.hip — k (tree id, leaf id) pairs anywhere in a built forest of trees of DIFFERENT sizes (forest_ragged.hip)
// proved by ONE shared proof and that proof checked with every ancestor hashed once, for both arities.  The proof is tree-major:
// P_0 | P_1 | .. | P_{n_trees - 1}, P_t byte for byte what multiproof.hip writes for tree t's block and tree t's positions, and
// proof_offsets[t] where P_t starts — a server cuts a tree's part out and hands it to a client of the single-tree verify.
// This is the segmented form of multiproof.hip's structure pass.  S_l is a list of (tree, node), sorted by both (the pairs are
// strictly ascending), so the elements of one tree and, inside it, of one parent are contiguous; every tree has its own width
// w_l^t = ceil(n_t / a^l), and an element whose tree has ONE node at level l is that tree's root: it opens no run and leaves the list.
//   k_fm_check       one lane per pair: tree id >= n_trees, a bad tree (n_t = 0 in the forest's index), leaf id >= n_t or not above
//                    its predecessor -> one count in *n_bad and the call's bad flag (every later kernel then leaves at once: nothing
//                    is read through a bad pair).  Writes S_0, the first pair of every tree, and for extraction gathers the leaves.
//   k_fm_tile_sums / k_fm_scan_tiles / k_fm_apply   one lane per element of S_l, tiles of 256 elements, a level of one tile skips
//                    the first two.  One device-wide scan carries two things: the heads (a change of (tree, parent)) counted
//                    across the whole list — the parent's place in S_{l+1} — and the heads' missing siblings counted PER TREE: the
//                    scan is segmented, it starts again at a tree's first element.  So a sibling's place is proof_offsets[t] + what
//                    tree t consumed at the levels below + the segmented sum, and the tree's new consumption is the sum at its last
//                    element: one lane per tree and level writes it, no atomic that the pairs of a tree share.  The consumption
//                    is double-buffered by level parity (the heads of a tree read it while its last element writes it).
//                    k_fm_apply writes per parent one 16-byte record in multiproof.hip's format, its tree and the width of the level
//                    below it, copies the missing siblings (extraction; 16-byte loads and stores, nothing at or past proof_cap)
//                    and deposits the value of a tree's root (verification).
//   k_fm_tree_sums / k_fm_tree_scan / k_fm_tree_offsets   extraction runs the structure pass twice: first counting only, then the
//                    exclusive scan of the per-tree totals over the trees (tiles of 2,048) = proof_offsets, then writing.
//   k_fm_finish_verify   one lane per tree: the verdict byte, the recomputed root (a one-leaf tree: its leaf reduced), the digest count
// Verification hashes through launch_multiproof_digest_list (multiproof.hip's k_mp_digest / k_mp_digest_coop on this unit's
// records): no kernel here runs the permutation.  ceil_shift, level_start, u64_of and the tree lookup are forest_node.hpp's.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_multiproof.h"
#include "forest_node.hpp"
#include "forest_ragged.h"
#include "multiproof.h"

namespace p252 {

namespace {

constexpr unsigned FM_BLOCK = 256;  // threads of a bookkeeping block = elements of a scan tile
constexpr unsigned FM_TREE_ITEMS = 8;
constexpr unsigned FM_TREE_TILE = FM_BLOCK * FM_TREE_ITEMS;  // trees per block of the scan over the trees
// the counters of one call (uint64 words): |S_l| for l = 0 .. 33, then
constexpr unsigned FM_BAD = 64;  // a bad pair was seen
constexpr size_t FM_COUNT_BYTES = 1024;
constexpr unsigned FM_MASK_SHIFT = 28;  // a record's last word: proof offset bits 32 .. 59, slot mask above (multiproof.hip's)
constexpr uint32_t FM_NONE = 0xffffffffu;  // no pair of the batch names this tree
// one element of the scan, packed: heads (a tile holds at most 256), the heads' missing siblings since the tree's first element
// (at most 3 x 256), and whether a tree starts at or before this element
constexpr unsigned FM_H = 0x3ffu, FM_M_SHIFT = 10, FM_M = 0xfffu << FM_M_SHIFT, FM_F = 1u << 31;

typedef unsigned long long u64;

// left then right: heads add up; the missing count starts again where a tree starts
__device__ __forceinline__ unsigned seg_combine(unsigned a, unsigned b) {
    const unsigned keep = (b & FM_F) ? 0u : (a & FM_M);
    return ((a & FM_H) + (b & (FM_H | FM_M)) + keep) | ((a | b) & FM_F);
}

// the combination of the threads BEFORE this one (0 for thread 0); *total = of the whole block
__device__ __forceinline__ unsigned block_seg_scan(unsigned v, unsigned* total) {
    __shared__ unsigned part[FM_BLOCK];
    const unsigned t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (unsigned off = 1; off < FM_BLOCK; off <<= 1) {
        const unsigned o = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] = seg_combine(o, part[t]);
        __syncthreads();
    }
    *total = part[FM_BLOCK - 1];
    const unsigned ex = t > 0 ? part[t - 1] : 0u;
    __syncthreads();  // (part is reused by the caller's next call)
    return ex;
}

}  // namespace

// S_l as the structure pass reads it: the nodes are level 0's own list (stride 1) or the first word of level l's records (stride 4)
struct FmLevel {
    const uint32_t* node;
    unsigned stride;
    const uint32_t* tree;   // the tree of every element
    const uint64_t* ntree;  // the forest's index: n_t
    unsigned shift;         // l * log2(arity): w_l^t = ceil(n_t / 2^shift)
    size_t lanes;           // the host's bound of |S_l|: the launch
};

struct FmElement {
    uint32_t tree, parent;
    unsigned mask;  // the child slots of the parent that S_l holds
    uint64_t w;     // nodes of level l of the element's tree
    bool dead;      // w == 1: the element is its tree's root
};

// element e of S_l (count elements) as the scan sees it: FM_F when its tree starts here; a head brings 1 and its parent's missing
// siblings
template <unsigned ARITY>
__device__ __forceinline__ unsigned fm_element(const FmLevel& L, uint64_t e, uint64_t count, FmElement& el) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    el.dead = false;
    if (e >= count) return 0;
    const uint32_t t = L.tree[e];
    const uint32_t pos = L.node[e * L.stride];
    const bool same_tree = e > 0 && L.tree[e - 1] == t;
    const unsigned flag = same_tree ? 0u : FM_F;
    el.tree = t;
    el.w = ceil_shift(L.ntree[t], L.shift);
    el.dead = el.w <= 1;
    if (el.dead) return flag;
    const uint32_t p = pos >> LA;
    if (same_tree && (L.node[(e - 1) * L.stride] >> LA) == p) return flag;
    unsigned m = 1u << (pos & (ARITY - 1));
#pragma unroll
    for (unsigned j = 1; j < ARITY; ++j) {
        if (e + j < count && L.tree[e + j] == t) {
            const uint32_t q = L.node[(e + j) * L.stride];
            if ((q >> LA) == p) m |= 1u << (q & (ARITY - 1));
        }
    }
    const uint64_t first = (uint64_t)p * ARITY;
    const unsigned present = first < el.w ? (unsigned)(el.w - first < ARITY ? el.w - first : ARITY) : 0u;
    const unsigned run = (unsigned)__popc(m);
    el.parent = p;
    el.mask = m;
    return flag | 1u | ((present > run ? present - run : 0u) << FM_M_SHIFT);
}

// ---- the pairs themselves ----
__global__ void __launch_bounds__(FM_BLOCK) k_fm_check(const uint64_t* __restrict__ ntree, size_t n_trees,
                                                       const uint32_t* __restrict__ tree_ids, const uint64_t* __restrict__ leaf_ids,
                                                       size_t k, const uint64_t* __restrict__ offsets, const uint4* __restrict__ leaves,
                                                       uint4* __restrict__ leaves_out, uint32_t* __restrict__ node0,
                                                       uint32_t* __restrict__ tree0, uint32_t* __restrict__ tfirst, u64* __restrict__ ctr,
                                                       unsigned* __restrict__ n_bad) {
    const size_t i = (size_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    if (i >= k) return;
    if (i == 0) ctr[0] = k;
    const uint32_t t = tree_ids[i];
    const uint64_t leaf = leaf_ids[i];
    size_t ts;
    const uint64_t n = forest_tree_leaves(ntree, n_trees, t, &ts);
    bool bad = n == 0 || leaf >= n;
    bool opens = true;  // the first pair of its tree
    if (i > 0) {
        const uint32_t tp = tree_ids[i - 1];
        const uint64_t lp = leaf_ids[i - 1];
        if (tp > t || (tp == t && lp >= leaf)) bad = true;
        opens = tp != t;
    }
    if (bad) {
        ctr[FM_BAD] = 1;
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    node0[i] = (uint32_t)leaf;  // (leaf < n_t <= max_leaves < 2^32)
    tree0[i] = t;
    if (tfirst && opens) tfirst[t] = (uint32_t)i;
    if (leaves) {  // (extraction)
        const size_t at = (size_t)(offsets[ts] + leaf);
        leaves_out[2 * i] = leaves[2 * at];
        leaves_out[2 * i + 1] = leaves[2 * at + 1];
    }
}

// ---- the structure pass l -> l + 1 ----
template <unsigned ARITY>
__global__ void __launch_bounds__(FM_BLOCK) k_fm_tile_sums(FmLevel L, const u64* __restrict__ ctr, unsigned l, uint32_t* __restrict__ tsum) {
    if (ctr[FM_BAD]) return;  // (the whole grid: S_0 is not written after a bad pair)
    const uint64_t e = (uint64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    FmElement el;
    const unsigned v = e < L.lanes ? fm_element<ARITY>(L, e, ctr[l], el) : 0u;
    unsigned total;
    (void)block_seg_scan(v, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one block: the tile sums -> toff[tile] = (heads before the tile, missing siblings of the tree that runs into the tile); |S_{l+1}|.
// FM_BLOCK tiles a trip of the loop: the second trip starts where a level's list is longer than FM_BLOCK * FM_BLOCK = 65,536 elements.
// `heads` adds up from trip to trip; `carry` (the missing siblings of the tree that runs out of the trip) restarts where a tree starts
__global__ void __launch_bounds__(FM_BLOCK) k_fm_scan_tiles(const uint32_t* __restrict__ tsum, size_t tiles, u64* __restrict__ toff,
                                                            u64* __restrict__ ctr, unsigned l) {
    if (ctr[FM_BAD]) return;
    __shared__ u64 ph[FM_BLOCK], pm[FM_BLOCK];
    __shared__ unsigned pf[FM_BLOCK];
    const unsigned t = threadIdx.x;
    u64 heads = 0, carry = 0;
#pragma unroll 1
    for (size_t at = 0; at < tiles; at += FM_BLOCK) {
        const size_t i = at + t;
        const uint32_t v = i < tiles ? tsum[i] : 0u;
        ph[t] = v & FM_H;
        pm[t] = (v & FM_M) >> FM_M_SHIFT;
        pf[t] = v >> 31;
        __syncthreads();
        for (unsigned off = 1; off < FM_BLOCK; off <<= 1) {
            const bool has = t >= off;
            const u64 oh = has ? ph[t - off] : 0ull, om = has ? pm[t - off] : 0ull;
            const unsigned of = has ? pf[t - off] : 0u;
            __syncthreads();
            ph[t] += oh;
            if (!pf[t]) pm[t] += om;
            pf[t] |= of;
            __syncthreads();
        }
        if (i < tiles) {
            toff[2 * i] = heads + (t > 0 ? ph[t - 1] : 0ull);
            const u64 em = t > 0 ? pm[t - 1] : 0ull;
            toff[2 * i + 1] = (t > 0 && pf[t - 1]) ? em : carry + em;
        }
        heads += ph[FM_BLOCK - 1];
        carry = pf[FM_BLOCK - 1] ? pm[FM_BLOCK - 1] : carry + pm[FM_BLOCK - 1];
        __syncthreads();  // (the lists are rewritten by the next chunk)
    }
    if (t == 0) ctr[l + 1] = heads;
}

// where the pass writes: level l + 1's work list, the per-tree consumption, and what each use of the pass adds
struct FmOut {
    uint4* rec;        // one record per parent (multiproof.hip's format), cap of them
    uint32_t* tree;    // its tree
    uint32_t* wnode;   // the width of level l of its tree (verification: the digests' child-slot rule), or null
    size_t cap;
    const u64* cons_in;  // scalars of tree t's part of the proof at the levels below l
    u64* cons_out;       // the same with level l
    u64* total;          // the latest of them: the tree's proof length once its last level is done
    const u64* base;     // proof_offsets (null: the counting pass), clamped to base_max
    u64 base_max;
    const uint4* vals;   // verification, l >= 1: the values of S_l — a root's is copied to rootval[t]
    uint4* rootval;
    // extraction
    const uint4* leaves;
    const uint4* levels;
    const uint64_t* offsets;
    const uint64_t* lo;
    uint4* proof;
    size_t proof_cap;
    unsigned level, la;
};

// toff == nullptr: the level is one tile, and this block does the whole scan
template <unsigned ARITY, bool EXTRACT>
__global__ void __launch_bounds__(FM_BLOCK) k_fm_apply(FmLevel L, FmOut O, u64* __restrict__ ctr, const u64* __restrict__ toff) {
    if (ctr[FM_BAD]) return;  // (the whole grid)
    const unsigned l = O.level;
    const uint64_t e = (uint64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    const uint64_t count = ctr[l];
    FmElement el;
    const unsigned v = e < L.lanes ? fm_element<ARITY>(L, e, count, el) : 0u;
    unsigned total;
    const unsigned ex = block_seg_scan(v, &total);
    u64 heads = 0, carry = 0;
    if (toff) {
        heads = toff[2 * (size_t)blockIdx.x];
        carry = toff[2 * (size_t)blockIdx.x + 1];
    } else if (threadIdx.x == 0) {
        ctr[l + 1] = total & FM_H;
    }
    if (e >= count || e >= L.lanes) return;
    const uint32_t t = el.tree;
    if (el.dead) {
        if (O.vals) {
            O.rootval[2 * (size_t)t] = O.vals[2 * e];
            O.rootval[2 * (size_t)t + 1] = O.vals[2 * e + 1];
        }
        return;
    }
    // the missing siblings of this tree's heads before this element
    const u64 before = (v & FM_F) ? 0ull : (u64)((ex & FM_M) >> FM_M_SHIFT) + ((ex & FM_F) ? 0ull : carry);
    const unsigned missing = (v & FM_M) >> FM_M_SHIFT;
    const u64 below = O.cons_in[t];
    if (e + 1 >= count || L.tree[e + 1] != t) {  // the tree's last element: one lane per tree
        O.cons_out[t] = below + before + missing;
        O.total[t] = below + before + missing;
    }
    if (!(v & FM_H)) return;
    const u64 place = heads + (ex & FM_H);
    u64 off = below + before;
    if (O.base) {
        const u64 b = O.base[t];
        off += b < O.base_max ? b : O.base_max;
    }
    if (place < O.cap) {
        O.rec[place] = make_uint4(el.parent, (unsigned)e, (unsigned)off, ((unsigned)(off >> 32) & ((1u << FM_MASK_SHIFT) - 1)) | (el.mask << FM_MASK_SHIFT));
        O.tree[place] = t;
        if (O.wnode) O.wnode[place] = (uint32_t)el.w;
    }
    if (EXTRACT) {
        // level l of tree t: its leaves, or its place inside the tree's block of the tree-major levels
        const uint4* src = l == 0 ? O.leaves + 2 * (size_t)O.offsets[t] : O.levels + 2 * (size_t)(O.lo[t] + level_start(L.ntree[t], l, O.la));
        const uint64_t first = (uint64_t)el.parent * ARITY;
#pragma unroll
        for (unsigned j = 0; j < ARITY; ++j) {
            const uint64_t c = first + j;
            if (c < el.w && !((el.mask >> j) & 1u)) {
                if (off < O.proof_cap) {
                    O.proof[2 * off] = src[2 * c];
                    O.proof[2 * off + 1] = src[2 * c + 1];
                }
                ++off;
            }
        }
    }
}

// ---- extraction: proof_offsets = the exclusive scan of the trees' totals (all zero after a bad pair: nothing was counted) ----
__global__ void __launch_bounds__(FM_BLOCK) k_fm_tree_sums(const u64* __restrict__ total, size_t n_trees, u64* __restrict__ ttile) {
    const size_t t0 = (size_t)blockIdx.x * FM_TREE_TILE + (size_t)threadIdx.x * FM_TREE_ITEMS;
    u64 sum = 0;
#pragma unroll
    for (unsigned q = 0; q < FM_TREE_ITEMS; ++q)
        if (t0 + q < n_trees) sum += total[t0 + q];
    u64 all;
    (void)block_exclusive<FM_BLOCK>(sum, &all);
    if (threadIdx.x == 0) ttile[blockIdx.x] = all;
}

// one block: the tree tiles' sums -> their exclusive scan, in place (scan_tile_row of blockops.hpp: the second trip of its loop starts
// past FM_BLOCK * FM_TREE_TILE = 524,288 trees)
__global__ void __launch_bounds__(FM_BLOCK) k_fm_tree_scan(u64* __restrict__ ttile, size_t tiles) {
    scan_tile_row<FM_BLOCK>(ttile, tiles);
}

// ttile == nullptr: one tile
__global__ void __launch_bounds__(FM_BLOCK) k_fm_tree_offsets(const u64* __restrict__ total, size_t n_trees, const u64* __restrict__ ttile,
                                                              u64* __restrict__ po) {
    const size_t t0 = (size_t)blockIdx.x * FM_TREE_TILE + (size_t)threadIdx.x * FM_TREE_ITEMS;
    u64 v[FM_TREE_ITEMS], sum = 0;
#pragma unroll
    for (unsigned q = 0; q < FM_TREE_ITEMS; ++q) {
        v[q] = t0 + q < n_trees ? total[t0 + q] : 0ull;
        sum += v[q];
    }
    u64 all;
    u64 run = (ttile ? ttile[blockIdx.x] : 0ull) + block_exclusive<FM_BLOCK>(sum, &all);
#pragma unroll
    for (unsigned q = 0; q < FM_TREE_ITEMS; ++q) {
        const size_t t = t0 + q;
        if (t >= n_trees) break;
        po[t] = run;
        run += v[q];
        if (t == n_trees - 1) po[n_trees] = run;
    }
}

// ---- verification: one lane per tree ----
__global__ void __launch_bounds__(FM_BLOCK) k_fm_finish_verify(const u64* __restrict__ ctr, unsigned depth, size_t n_trees,
                                                               const uint64_t* __restrict__ ntree, const uint32_t* __restrict__ tfirst,
                                                               const u64* __restrict__ total, const u64* __restrict__ po, uint64_t proof_len,
                                                               const uint4* __restrict__ rootval, const Scalar32* __restrict__ leaves_in,
                                                               const uint4* __restrict__ roots, uint8_t* __restrict__ ok,
                                                               uint4* __restrict__ roots_out, u64* __restrict__ n_hashed) {
    const size_t t = (size_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    const bool bad = ctr[FM_BAD] != 0;
    if (t == 0 && n_hashed) {
        u64 hashed = 0;
        for (unsigned l = 1; l <= depth; ++l) hashed += ctr[l];
        *n_hashed = bad ? 0ull : hashed;
    }
    if (t >= n_trees) return;
    const uint32_t first = tfirst[t];
    bool whole = !bad && first != FM_NONE;
    if (whole) {
        const u64 a = po[t], b = po[t + 1];
        whole = a <= b && b <= proof_len && total[t] == b - a;
    }
    bool same = false;
    if (whole) {
        uint4 lo, hi;
        if (ntree[t] == 1) {  // the forest's convention: a one-leaf tree's root is its leaf mod p
            uint32_t w[8];
            to_mont4(load_scalar(leaves_in + first), w);
            lo = make_uint4(w[0], w[1], w[2], w[3]);
            hi = make_uint4(w[4], w[5], w[6], w[7]);
        } else {
            lo = rootval[2 * t];
            hi = rootval[2 * t + 1];
        }
        const uint4 rlo = roots[2 * t], rhi = roots[2 * t + 1];
        same = lo.x == rlo.x && lo.y == rlo.y && lo.z == rlo.z && lo.w == rlo.w && hi.x == rhi.x && hi.y == rhi.y && hi.z == rhi.z &&
               hi.w == rhi.w;
        if (roots_out) {
            roots_out[2 * t] = lo;
            roots_out[2 * t + 1] = hi;
        }
    }
    ok[t] = same ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
namespace {

size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// the scratch of one call, carved out of `work` behind the forest's index
struct FmWork {
    u64 *ctr, *cons[2], *total, *ttile, *toff;
    uint32_t *tfirst, *tsum, *node0, *tree0, *tree[2], *wnode;  // (S_0 keeps its own lists: extraction reads them twice)
    uint4 *rootval, *rec[2];
    size_t zero_bytes;  // the counters, both consumptions and the totals, contiguous from ctr
};
FmWork fm_work(const ForestMultiproofPlan& p, void* work) {
    char* b = static_cast<char*>(work) + p.index_bytes;
    const size_t T = p.n_trees, k = p.k;
    FmWork w;
    auto take = [&](size_t bytes) {
        char* at = b;
        b += round256(bytes);
        return at;
    };
    w.ctr = reinterpret_cast<u64*>(b);
    w.zero_bytes = round256(FM_COUNT_BYTES + 3 * T * 8);
    char* z = take(FM_COUNT_BYTES + 3 * T * 8);
    w.cons[0] = reinterpret_cast<u64*>(z + FM_COUNT_BYTES);
    w.cons[1] = w.cons[0] + T;
    w.total = w.cons[1] + T;
    w.tfirst = reinterpret_cast<uint32_t*>(take(T * 4));
    w.rootval = reinterpret_cast<uint4*>(take(T * 32));
    w.ttile = reinterpret_cast<u64*>(take(p.tree_tiles * 8));
    w.tsum = reinterpret_cast<uint32_t*>(take(p.tiles * 4));
    w.toff = reinterpret_cast<u64*>(take(p.tiles * 16));
    w.node0 = reinterpret_cast<uint32_t*>(take(k * 4));
    w.tree0 = reinterpret_cast<uint32_t*>(take(k * 4));
    w.tree[0] = reinterpret_cast<uint32_t*>(take(k * 4));
    w.tree[1] = reinterpret_cast<uint32_t*>(take(k * 4));
    w.wnode = reinterpret_cast<uint32_t*>(take(k * 4));
    w.rec[0] = reinterpret_cast<uint4*>(take(k * 16));
    w.rec[1] = reinterpret_cast<uint4*>(take(k * 16));
    return w;
}

// the structure pass l -> l + 1: S_l = level 0's own lists (l == 0) or rec / tree [l & 1]; the records of S_{l+1} to rec / tree [(l + 1) & 1]
template <unsigned ARITY, bool EXTRACT>
hipError_t fm_step(const ForestMultiproofPlan& p, const FmWork& w, const uint64_t* ntree, unsigned l, FmOut O, hipStream_t st) {
    FmLevel L;
    L.node = l == 0 ? w.node0 : reinterpret_cast<const uint32_t*>(w.rec[l & 1]);
    L.stride = l == 0 ? 1 : 4;
    L.tree = l == 0 ? w.tree0 : w.tree[l & 1];
    L.ntree = ntree;
    L.shift = l * p.log2a;
    L.lanes = p.in[l];
    O.rec = w.rec[(l + 1) & 1];
    O.tree = w.tree[(l + 1) & 1];
    O.cap = p.k;
    O.cons_in = w.cons[l & 1];
    O.cons_out = w.cons[(l + 1) & 1];
    O.total = w.total;
    O.rootval = w.rootval;
    O.level = l;
    O.la = p.log2a;
    const unsigned tiles = (unsigned)((L.lanes + FM_BLOCK - 1) / FM_BLOCK);
    const dim3 blk(FM_BLOCK);
    if (tiles > 1) {
        hipLaunchKernelGGL(k_fm_tile_sums<ARITY>, dim3(tiles), blk, 0, st, L, w.ctr, l, w.tsum);
        hipLaunchKernelGGL(k_fm_scan_tiles, dim3(1), blk, 0, st, w.tsum, (size_t)tiles, w.toff, w.ctr, l);
    }
    hipLaunchKernelGGL((k_fm_apply<ARITY, EXTRACT>), dim3(tiles), blk, 0, st, L, O, w.ctr, tiles > 1 ? w.toff : (const u64*)nullptr);
    return hipGetLastError();
}

template <bool EXTRACT>
hipError_t fm_step_arity(const ForestMultiproofPlan& p, const FmWork& w, const uint64_t* ntree, unsigned l, const FmOut& O, hipStream_t st) {
    return p.arity == 4 ? fm_step<4, EXTRACT>(p, w, ntree, l, O, st) : fm_step<2, EXTRACT>(p, w, ntree, l, O, st);
}

}  // namespace

ForestMultiproofPlan forest_multiproof_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k) {
    ForestMultiproofPlan p;
    p.arity = arity;
    p.log2a = arity == 4 ? 2 : 1;
    p.k = k;
    p.n_trees = n_trees;
    p.n_leaves = n_leaves;
    p.max_leaves = max_leaves;
    if (k == 0 || n_trees == 0 || n_leaves == 0 || max_leaves == 0) return p;
    const unsigned full = forest_ragged_depth(max_leaves, arity);  // D of the bound
    p.depth = forest_ragged_depth(max_leaves < n_leaves ? max_leaves : n_leaves, arity);  // no good tree is deeper
    if (p.depth > FOREST_MULTIPROOF_MAX_DEPTH) p.depth = FOREST_MULTIPROOF_MAX_DEPTH;     // (api.cpp refuses max_leaves >= 2^32)
    p.in[0] = k;
    for (unsigned l = 1; l <= p.depth + 1; ++l) {
        const size_t width = (n_leaves >> (l * p.log2a)) + n_trees;
        p.in[l] = k < width ? k : width;
    }
    const size_t per_pair = (size_t)full * (arity - 1);
    const size_t by_pairs = k > SIZE_MAX / (per_pair ? per_pair : 1) ? SIZE_MAX : k * per_pair;
    const size_t by_nodes = n_leaves + n_leaves / (arity - 1) + n_trees * full;
    p.bound = by_pairs < by_nodes ? by_pairs : by_nodes;
    p.tiles = (k + FM_BLOCK - 1) / FM_BLOCK;
    p.tree_tiles = (n_trees + FM_TREE_TILE - 1) / FM_TREE_TILE;
    p.index_bytes = forest_ragged_index_bytes(n_trees);
    p.tree_bytes = round256(FM_COUNT_BYTES + 3 * n_trees * 8) + round256(n_trees * 4) + round256(n_trees * 32) + round256(p.tree_tiles * 8);
    p.pair_bytes = round256(p.tiles * 4) + round256(p.tiles * 16) + 5 * round256(k * 4) + 2 * round256(k * 16);
    return p;
}

hipError_t launch_forest_multiproof(const ForestMultiproofPlan& p, const void* leaves, const void* offsets, const void* levels,
                                    const void* tree_ids, const void* leaf_ids, void* leaves_out, void* proof, size_t proof_cap,
                                    void* proof_offsets, void* n_bad, void* work, hipStream_t st) {
    const FmWork w = fm_work(p, work);
    const uint64_t *ntree = nullptr, *lo = nullptr;
    hipError_t e = launch_forest_ragged_index(p.arity, offsets, p.n_trees, p.n_leaves, p.max_leaves, work, &ntree, &lo, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.ctr, 0, w.zero_bytes, st);
    if (e != hipSuccess) return e;
    const dim3 blk(FM_BLOCK);
    hipLaunchKernelGGL(k_fm_check, dim3((unsigned)((p.k + FM_BLOCK - 1) / FM_BLOCK)), blk, 0, st, ntree, p.n_trees,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint64_t*>(leaf_ids), p.k,
                       static_cast<const uint64_t*>(offsets), static_cast<const uint4*>(leaves), static_cast<uint4*>(leaves_out), w.node0,
                       w.tree0, (uint32_t*)nullptr, w.ctr, static_cast<unsigned*>(n_bad));
    e = hipGetLastError();
    // the counting pass: every tree's total
    FmOut O = {};
    for (unsigned l = 0; l < p.depth && e == hipSuccess; ++l) e = fm_step_arity<false>(p, w, ntree, l, O, st);
    if (e != hipSuccess) return e;
    u64* po = static_cast<u64*>(proof_offsets);
    const unsigned tt = (unsigned)p.tree_tiles;
    if (tt > 1) {
        hipLaunchKernelGGL(k_fm_tree_sums, dim3(tt), blk, 0, st, w.total, p.n_trees, w.ttile);
        hipLaunchKernelGGL(k_fm_tree_scan, dim3(1), blk, 0, st, w.ttile, (size_t)tt);
    }
    hipLaunchKernelGGL(k_fm_tree_offsets, dim3(tt), blk, 0, st, w.total, p.n_trees, tt > 1 ? w.ttile : (const u64*)nullptr, po);
    e = hipGetLastError();
    if (e != hipSuccess || p.depth == 0) return e;
    // the writing pass: the same structure again, every sibling to its place behind proof_offsets[t]
    e = hipMemsetAsync(w.cons[0], 0, 2 * p.n_trees * 8, st);
    O.base = po;
    O.base_max = ~0ull;
    O.leaves = static_cast<const uint4*>(leaves);
    O.levels = static_cast<const uint4*>(levels);
    O.offsets = static_cast<const uint64_t*>(offsets);
    O.lo = lo;
    O.proof = static_cast<uint4*>(proof);
    O.proof_cap = proof_cap;
    for (unsigned l = 0; l < p.depth && e == hipSuccess; ++l) e = fm_step_arity<true>(p, w, ntree, l, O, st);
    return e;
}

hipError_t launch_forest_multiproof_verify(const int32_t* tab, const TagArg& tag, const ForestMultiproofPlan& p, const void* offsets,
                                           const void* tree_ids, const void* leaf_ids, const void* leaves_in, const void* proof,
                                           size_t proof_len, const void* proof_offsets, const void* roots, void* ok, void* roots_out,
                                           void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st) {
    const FmWork w = fm_work(p, work);
    const uint64_t *ntree = nullptr, *lo = nullptr;
    hipError_t e = launch_forest_ragged_index(p.arity, offsets, p.n_trees, p.n_leaves, p.max_leaves, work, &ntree, &lo, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.ctr, 0, w.zero_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.tfirst, 0xff, p.n_trees * 4, st);
    if (e != hipSuccess) return e;
    const dim3 blk(FM_BLOCK);
    hipLaunchKernelGGL(k_fm_check, dim3((unsigned)((p.k + FM_BLOCK - 1) / FM_BLOCK)), blk, 0, st, ntree, p.n_trees,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint64_t*>(leaf_ids), p.k, (const uint64_t*)nullptr,
                       (const uint4*)nullptr, (uint4*)nullptr, w.node0, w.tree0, w.tfirst, w.ctr, static_cast<unsigned*>(n_bad));
    e = hipGetLastError();
    Scalar32* vals[2] = {static_cast<Scalar32*>(values), static_cast<Scalar32*>(values) + p.k};
    FmOut O = {};
    O.wnode = w.wnode;
    O.base = static_cast<const u64*>(proof_offsets);
    O.base_max = proof_len;
    // level `depth` has roots only: its pass deposits them and makes no list
    for (unsigned l = 0; l <= p.depth && e == hipSuccess; ++l) {
        O.vals = l == 0 ? nullptr : reinterpret_cast<const uint4*>(vals[l & 1]);
        e = fm_step_arity<false>(p, w, ntree, l, O, st);
        if (e != hipSuccess || l == p.depth) break;
        MultiproofDigestList d;
        d.list = w.rec[(l + 1) & 1];
        d.count = w.ctr + (l + 1);
        d.vals_in = l == 0 ? leaves_in : static_cast<const void*>(vals[l & 1]);
        d.vals_out = vals[(l + 1) & 1];
        d.proof = proof;
        d.proof_len = proof_len;
        d.w_node = w.wnode;
        d.bound = p.in[l + 1];
        e = launch_multiproof_digest_list(tab, tag, p.arity, d, st);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fm_finish_verify, dim3((unsigned)((p.n_trees + FM_BLOCK - 1) / FM_BLOCK)), blk, 0, st, w.ctr, p.depth, p.n_trees,
                       ntree, w.tfirst, w.total, static_cast<const u64*>(proof_offsets), (uint64_t)proof_len, w.rootval,
                       static_cast<const Scalar32*>(leaves_in), static_cast<const uint4*>(roots), static_cast<uint8_t*>(ok),
                       static_cast<uint4*>(roots_out), static_cast<u64*>(n_hashed));
    return hipGetLastError();
}

}  // namespace p252
