// multiproof.hip — k leaves of ONE stored tree (kernels.hip's builder, or one tree block of a ragged forest: the same layout) proved
// by one shared proof, and that proof checked with every ancestor hashed ONCE, for both arities.  The per-leaf openings
// (openings.hip) write depth x (arity - 1) siblings per leaf and their verification re-hashes k x depth nodes; here a sibling that
// another leaf of the batch determines is never stored and an ancestor that several leaves share is hashed by one lane.
// The format (include/poseidon252_hip.h): positions strictly ascending; S_0 = the positions, S_{l+1} = the distinct
// parents of S_l; level by level, parent by parent, child slot by child slot, the proof holds every child that exists (< w_l) and
// is not in S_l.  Sorted input makes S_l a sorted list whose equal-parent runs are contiguous, so one step l -> l + 1 is a scan:
//   k_mp_check       one lane per position: >= n_leaves or not above its predecessor -> one count in *n_bad and the call's bad
//                    flag (every later kernel then leaves at once: nothing is read through a bad position); extraction also
//                    gathers the leaves here
//   k_mp_tile_sums / k_mp_scan_tiles / k_mp_apply   the structure pass, one lane per element of S_l.  An element that opens its
//                    parent's run is a head: it reads the run (at most arity elements), knows which child slots are present and
//                    how many siblings are missing.  An exclusive device-wide scan (three passes over tiles of 256 elements, after
//                    forest_ragged.hip's) of the heads gives the parent's place in S_{l+1}, of the missing counts its offset in the
//                    proof; the level's proof base accumulates in a device counter, and |S_{l+1}| is left on the device too: the
//                    launches are sized by the host bound min(k, w_l).  A level of one tile skips the first two passes.
//                    k_mp_apply writes one 16-byte record per parent (parent index, start of its run in S_l, proof offset, slot
//                    mask) — the work list of level l + 1 — and, for extraction, copies the missing siblings out of the stored level
//                    (16-byte loads and stores; nothing at or past proof_cap).
//   k_mp_digest / k_mp_digest_coop   verification: lane (group of 8 lanes) g < |S_{l+1}| hashes record g: each child from level l's
//                    value list (the leaves for l = 0), from the proof stream (zero at or past proof_len: the length check fails
//                    the proof anyway) or zero, the digest to level l + 1's value list.  As k_fu_digest / k_fu_digest_coop:
//                    hades_permute<0x02u, true> with the hoisted tag S-box at 3 waves per SIMD, node_digest_coop when the level
//                    cannot fill the chip (coop8 of the host bound).
//   k_mp_finish_*    the proof length; or the one-byte verdict: no bad position, exactly proof_len scalars consumed, root equal.
// launch_multiproof_digest_list runs the two digest kernels over records that another unit made (forest_multiproof.hip: the shared
// proof across a ragged forest); there every record belongs to a tree of its own size, so the number of child slots that exist is
// read per record (MpDigest::w_node) instead of once per launch (w_below; w_node == null: this file's own calls).
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_node.hpp"
#include "hades29.hpp"
#include "kernels.h"
#include "multiproof.h"

namespace p252 {

namespace {

constexpr unsigned MP_BLOCK = 256;  // threads of a bookkeeping block = elements of a scan tile
// the counters of one call (uint64 words): |S_l| for l = 0 .. 32, then
constexpr unsigned MP_BASE = MULTIPROOF_MAX_DEPTH + 1;  // proof scalars of the levels done so far
constexpr unsigned MP_BAD = MULTIPROOF_MAX_DEPTH + 2;   // a bad position was seen
constexpr size_t MP_COUNT_BYTES = 512;
constexpr unsigned MP_MASK_SHIFT = 28;  // a record's last word: proof offset bits 32 .. 59, slot mask above

typedef unsigned long long u64;

}  // namespace

// S_l as the structure pass reads it: the caller's positions (stride 1) or the first word of level l's records (stride 4)
struct MpLevel {
    const uint32_t* in;
    unsigned stride;
    uint64_t w;    // nodes of level l
    size_t lanes;  // min(k, w): the launch
};

// element e of S_l (count elements): 0 unless it opens its parent's run, else 1 << 16 | the parent's missing siblings, with the
// parent and the mask of the child slots that S_l holds
template <unsigned ARITY>
__device__ __forceinline__ unsigned mp_element(const MpLevel& L, uint64_t e, uint64_t count, uint32_t* parent, unsigned* mask) {
    constexpr unsigned LA = ARITY == 4 ? 2 : 1;
    if (e >= count) return 0;
    const uint32_t pos = L.in[e * L.stride];
    const uint32_t p = pos >> LA;
    if (e > 0 && (L.in[(e - 1) * L.stride] >> LA) == p) return 0;
    unsigned m = 1u << (pos & (ARITY - 1));
#pragma unroll
    for (unsigned t = 1; t < ARITY; ++t) {
        if (e + t < count) {
            const uint32_t q = L.in[(e + t) * L.stride];
            if ((q >> LA) == p) m |= 1u << (q & (ARITY - 1));
        }
    }
    const uint64_t first = (uint64_t)p * ARITY;
    const unsigned present = first < L.w ? (unsigned)(L.w - first < ARITY ? L.w - first : ARITY) : 0u;
    const unsigned run = (unsigned)__popc(m);
    *parent = p;
    *mask = m;
    return 0x10000u | (present > run ? present - run : 0u);
}

// ---- the positions themselves ----
__global__ void __launch_bounds__(MP_BLOCK) k_mp_check(const uint32_t* __restrict__ index, size_t k, uint64_t n_leaves,
                                                       const uint4* __restrict__ leaves, uint4* __restrict__ leaves_out,
                                                       u64* __restrict__ ctr, unsigned* __restrict__ n_bad) {
    const size_t e = (size_t)blockIdx.x * MP_BLOCK + threadIdx.x;
    if (e >= k) return;
    if (e == 0) ctr[0] = k;
    const uint32_t pos = index[e];
    if (pos >= n_leaves || (e > 0 && pos <= index[e - 1])) {
        ctr[MP_BAD] = 1;
        if (n_bad) atomicAdd(n_bad, 1u);
    } else if (leaves) {  // (extraction)
        leaves_out[2 * e] = leaves[2 * (size_t)pos];
        leaves_out[2 * e + 1] = leaves[2 * (size_t)pos + 1];
    }
}

// ---- the structure pass l -> l + 1 ----
template <unsigned ARITY>
__global__ void __launch_bounds__(MP_BLOCK) k_mp_tile_sums(MpLevel L, const u64* __restrict__ ctr, unsigned l, uint32_t* __restrict__ tsum) {
    const uint64_t e = (uint64_t)blockIdx.x * MP_BLOCK + threadIdx.x;
    uint32_t p;
    unsigned mask;
    const unsigned v = e < L.lanes ? mp_element<ARITY>(L, e, ctr[l], &p, &mask) : 0u;
    unsigned total;
    (void)block_exclusive<MP_BLOCK>(v, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one block: the tile sums -> toff[tile] = (heads before the tile, proof offset of the tile); the level's totals to the counters.
// MP_BLOCK tiles a trip of the loop, `heads` and `base` carried from trip to trip: the second trip starts where a level's list is
// longer than MP_BLOCK * MP_BLOCK = 65,536 elements
__global__ void __launch_bounds__(MP_BLOCK) k_mp_scan_tiles(const uint32_t* __restrict__ tsum, size_t tiles, u64* __restrict__ toff,
                                                            u64* __restrict__ ctr, unsigned l) {
    u64 heads = 0, base = ctr[MP_BASE];
#pragma unroll 1
    for (size_t at = 0; at < tiles; at += MP_BLOCK) {
        const size_t i = at + threadIdx.x;
        const uint32_t v = i < tiles ? tsum[i] : 0u;
        u64 th, tm;
        const u64 eh = block_exclusive<MP_BLOCK, u64>(v >> 16, &th);
        const u64 em = block_exclusive<MP_BLOCK, u64>(v & 0xffffu, &tm);
        if (i < tiles) {
            toff[2 * i] = heads + eh;
            toff[2 * i + 1] = base + em;
        }
        heads += th;
        base += tm;
    }
    __syncthreads();  // (every thread has read the old base)
    if (threadIdx.x == 0 && !ctr[MP_BAD]) {
        ctr[l + 1] = heads;
        ctr[MP_BASE] = base;
    }
}

// toff == nullptr: the level is one tile, and this block does the whole scan
template <unsigned ARITY, bool EXTRACT>
__global__ void __launch_bounds__(MP_BLOCK) k_mp_apply(MpLevel L, u64* __restrict__ ctr, unsigned l, const u64* __restrict__ toff,
                                                       uint4* __restrict__ out, size_t out_cap, const uint4* __restrict__ src,
                                                       uint4* __restrict__ proof, size_t proof_cap) {
    if (ctr[MP_BAD]) return;  // (the whole grid)
    const uint64_t e = (uint64_t)blockIdx.x * MP_BLOCK + threadIdx.x;
    uint32_t p = 0;
    unsigned mask = 0;
    const unsigned v = e < L.lanes ? mp_element<ARITY>(L, e, ctr[l], &p, &mask) : 0u;
    unsigned total;
    const unsigned ex = block_exclusive<MP_BLOCK>(v, &total);
    u64 heads = 0, base;
    if (toff) {
        heads = toff[2 * (size_t)blockIdx.x];
        base = toff[2 * (size_t)blockIdx.x + 1];
    } else {
        base = ctr[MP_BASE];
        __syncthreads();  // (every thread has read the old base)
        if (threadIdx.x == 0) {
            ctr[l + 1] = total >> 16;
            ctr[MP_BASE] = base + (total & 0xffffu);
        }
    }
    if (!(v >> 16)) return;
    const u64 place = heads + (ex >> 16);
    u64 off = base + (ex & 0xffffu);
    if (place < out_cap) out[place] = make_uint4(p, (unsigned)e, (unsigned)off, (unsigned)(off >> 32) | (mask << MP_MASK_SHIFT));
    if (EXTRACT) {
        const uint64_t first = (uint64_t)p * ARITY;
#pragma unroll
        for (unsigned j = 0; j < ARITY; ++j) {
            const uint64_t c = first + j;
            if (c < L.w && !((mask >> j) & 1u)) {
                if (off < proof_cap) {
                    proof[2 * off] = src[2 * c];
                    proof[2 * off + 1] = src[2 * c + 1];
                }
                ++off;
            }
        }
    }
}

__global__ void k_mp_finish_extract(const u64* __restrict__ ctr, u64* __restrict__ proof_len) {
    *proof_len = ctr[MP_BAD] ? 0ull : ctr[MP_BASE];
}

// ---- the digests of level l + 1 ----
struct MpDigest {
    const uint4* list;         // this level's records
    const u64* count;          // how many
    const Scalar32* vals_in;   // the values of S_l, in its order
    Scalar32* vals_out;        // the values of S_{l+1}
    const Scalar32* proof;
    uint64_t proof_len;
    uint64_t w_below;          // nodes of level l
    const uint32_t* w_node;    // null, or the nodes of level l PER RECORD (a forest: every record has its own tree) instead of w_below
    size_t lanes;
};

struct MpNode {
    uint64_t first, run, off;  // first child slot; the run's start in S_l; the node's offset in the proof
    uint64_t w;                // nodes of the level below: child slots at or past it do not exist
    unsigned mask;
};
__device__ __forceinline__ bool mp_node(const MpDigest& P, uint64_t g, unsigned arity, MpNode& nd) {
    if (g >= *P.count) return false;
    const uint4 r = P.list[g];
    nd.first = (uint64_t)r.x * arity;
    nd.run = r.y;
    nd.mask = r.w >> MP_MASK_SHIFT;
    nd.off = u64_of(r.z, r.w & ((1u << MP_MASK_SHIFT) - 1));
    nd.w = P.w_node ? (uint64_t)P.w_node[g] : P.w_below;
    return true;
}
// where child slot j of the node comes from: level l's values, the proof, or nowhere (null: zero)
template <unsigned ARITY>
__device__ __forceinline__ const Scalar32* mp_child(const MpDigest& P, const MpNode& nd, unsigned j) {
    if (j >= ARITY || nd.first + j >= nd.w) return nullptr;
    const unsigned below = (unsigned)__popc(nd.mask & ((1u << j) - 1u));  // slots before j that S_l holds
    if ((nd.mask >> j) & 1u) return P.vals_in + nd.run + below;
    const uint64_t at = nd.off + (j - below);
    return at < P.proof_len ? P.proof + at : nullptr;
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_mp_digest(const int32_t* __restrict__ tab, TagArg tag, MpDigest P) {
    const uint64_t g = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (g >= P.lanes) return;
    MpNode nd;
    if (!mp_node(P, g, ARITY, nd)) return;
    E29 s[WIDTH];  // (written out, as in k_fu_digest)
#pragma unroll
    for (int k = 0; k < NL; ++k) s[0].d[k] = tag.x0[k];  // lane 0 enters after its first S-box (hades_permute PRE0)
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const Scalar32* c = mp_child<ARITY>(P, nd, k);
        if (c)
            s[1 + k] = load_scalar(c);
        else
            s[1 + k] = e29_zero();
    }
    hades_permute<0x02u, true>(s, tab);  // only lane 1 is squeezed
    store_scalar(P.vals_out + g, s[1]);
}

template <unsigned ARITY>
__global__ void __launch_bounds__(P252_BLOCK) k_mp_digest_coop(const int32_t* __restrict__ tab, TagArg tag, MpDigest P) {
    const uint64_t lane = (uint64_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (lane >= P.lanes) return;  // (lanes is a multiple of 8: whole groups only)
    MpNode nd;
    if (!mp_node(P, lane >> 3, ARITY, nd)) return;  // (the whole group: one node)
    const int j = (int)(threadIdx.x & 7u);
    // node_digest_coop reads element el >= 1 of the state at children[ARITY i + el - 1]: each lane hands it its own child as a
    // one-node level (i = 0) that starts el - 1 scalars before that child, or an empty level (n_children = 0) for a zero
    const int el = j < WIDTH ? j : WIDTH - 1;
    const Scalar32* c = el > 0 ? mp_child<ARITY>(P, nd, (unsigned)(el - 1)) : nullptr;
    const E29 mine = node_digest_coop<ARITY>(tab, tag, c ? c - (el - 1) : P.vals_in, 0, c ? ARITY : 0, j);
    if (j == 1) store_scalar(P.vals_out + (lane >> 3), mine);  // the digest is element 1 of the permuted state: lane 1's
}

__global__ void k_mp_finish_verify(const u64* __restrict__ ctr, unsigned depth, uint64_t proof_len, const uint4* __restrict__ value,
                                   const uint4* __restrict__ root, uint8_t* __restrict__ ok, uint4* __restrict__ root_out,
                                   u64* __restrict__ n_hashed) {
    const bool bad = ctr[MP_BAD] != 0;
    const bool whole = !bad && ctr[MP_BASE] == proof_len && ctr[depth] == 1;  // (one node on top: the root)
    u64 hashed = 0;
    for (unsigned l = 1; l <= depth; ++l) hashed += ctr[l];
    if (n_hashed) *n_hashed = hashed;
    bool same = false;
    if (whole) {
        const uint4 lo = value[0], hi = value[1], rlo = root[0], rhi = root[1];
        same = lo.x == rlo.x && lo.y == rlo.y && lo.z == rlo.z && lo.w == rlo.w && hi.x == rhi.x && hi.y == rhi.y && hi.z == rhi.z &&
               hi.w == rhi.w;
        if (root_out) {
            root_out[0] = lo;
            root_out[1] = hi;
        }
    }
    *ok = same ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
namespace {

size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// the scratch of one call, carved out of `work`
struct MpWork {
    u64* ctr;
    u64* toff;
    uint32_t* tsum;
    uint4* list[2];
};
MpWork mp_work(const MultiproofPlan& p, void* work) {
    char* b = static_cast<char*>(work);
    MpWork w;
    w.ctr = reinterpret_cast<u64*>(b);
    w.toff = reinterpret_cast<u64*>(b + p.count_bytes);
    w.tsum = reinterpret_cast<uint32_t*>(b + p.count_bytes + round256(p.tiles * 16));
    w.list[0] = reinterpret_cast<uint4*>(b + p.count_bytes + p.tile_bytes);
    w.list[1] = reinterpret_cast<uint4*>(b + p.count_bytes + p.tile_bytes + p.list_bytes);
    return w;
}

hipError_t mp_begin(const MultiproofPlan& p, const MpWork& w, const void* indices, const void* leaves, void* leaves_out, void* n_bad,
                    hipStream_t st) {
    hipError_t e = hipMemsetAsync(w.ctr, 0, p.count_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mp_check, dim3((unsigned)((p.k + MP_BLOCK - 1) / MP_BLOCK)), dim3(MP_BLOCK), 0, st,
                       static_cast<const uint32_t*>(indices), p.k, (uint64_t)p.w[0], static_cast<const uint4*>(leaves),
                       static_cast<uint4*>(leaves_out), w.ctr, static_cast<unsigned*>(n_bad));
    return hipGetLastError();
}

// the structure pass l -> l + 1: S_l = the positions (l == 0) or list[l & 1], the records of S_{l+1} to list[(l + 1) & 1]
template <unsigned ARITY, bool EXTRACT>
hipError_t mp_step(const MultiproofPlan& p, const MpWork& w, unsigned l, const void* indices, const void* src, void* proof,
                   size_t proof_cap, hipStream_t st) {
    MpLevel L;
    L.in = l == 0 ? static_cast<const uint32_t*>(indices) : reinterpret_cast<const uint32_t*>(w.list[l & 1]);
    L.stride = l == 0 ? 1 : 4;
    L.w = p.w[l];
    L.lanes = p.in[l];
    const unsigned tiles = (unsigned)((L.lanes + MP_BLOCK - 1) / MP_BLOCK);
    const dim3 blk(MP_BLOCK);
    if (tiles > 1) {
        hipLaunchKernelGGL(k_mp_tile_sums<ARITY>, dim3(tiles), blk, 0, st, L, w.ctr, l, w.tsum);
        hipLaunchKernelGGL(k_mp_scan_tiles, dim3(1), blk, 0, st, w.tsum, (size_t)tiles, w.toff, w.ctr, l);
    }
    hipLaunchKernelGGL((k_mp_apply<ARITY, EXTRACT>), dim3(tiles), blk, 0, st, L, w.ctr, l, tiles > 1 ? w.toff : (const u64*)nullptr,
                       w.list[(l + 1) & 1], p.in[l + 1], static_cast<const uint4*>(src), static_cast<uint4*>(proof), proof_cap);
    return hipGetLastError();
}

// one level's digests: the 8-lane kernel when the level's host bound cannot fill the chip (the coop8 rule of kernels.h)
hipError_t mp_digests(const int32_t* tab, const TagArg& tag, unsigned arity, MpDigest& P, size_t bound, hipStream_t st) {
    const bool coop = coop8(bound);
    P.lanes = coop ? bound * 8 : bound;
    if (arity == 4) return launch(coop ? k_mp_digest_coop<4> : k_mp_digest<4>, P.lanes, st, tab, tag, P);
    return launch(coop ? k_mp_digest_coop<2> : k_mp_digest<2>, P.lanes, st, tab, tag, P);
}

}  // namespace

// the same over a record list made by the caller (forest_multiproof.hip): every record brings the width of the level below it
hipError_t launch_multiproof_digest_list(const int32_t* tab, const TagArg& tag, unsigned arity, const MultiproofDigestList& d,
                                         hipStream_t st) {
    if (d.bound == 0) return hipSuccess;
    MpDigest P;
    P.list = static_cast<const uint4*>(d.list);
    P.count = d.count;
    P.vals_in = static_cast<const Scalar32*>(d.vals_in);
    P.vals_out = static_cast<Scalar32*>(d.vals_out);
    P.proof = static_cast<const Scalar32*>(d.proof);
    P.proof_len = d.proof_len;
    P.w_below = 0;
    P.w_node = d.w_node;
    return mp_digests(tab, tag, arity, P, d.bound, st);
}

MultiproofPlan multiproof_plan(unsigned arity, size_t n_leaves, size_t k) {
    MultiproofPlan p;
    p.arity = arity;
    p.log2a = arity == 4 ? 2 : 1;
    p.k = k;
    p.w[0] = n_leaves;
    p.in[0] = k < n_leaves ? k : n_leaves;
    while (p.w[p.depth] > 1 && p.depth < MULTIPROOF_MAX_DEPTH) {
        const unsigned l = p.depth++;
        p.w[l + 1] = (p.w[l] + arity - 1) / arity;
        p.start[l + 1] = l == 0 ? 0 : p.start[l] + p.w[l];
        p.in[l + 1] = k < p.w[l + 1] ? k : p.w[l + 1];
        const size_t by_parents = (arity - 1) * p.in[l + 1], by_width = p.w[l] - p.in[l];
        p.bound += by_parents < by_width ? by_parents : by_width;
    }
    p.in[0] = k;  // (the check and level 0's pass see every position, good or not)
    p.tiles = (k + MP_BLOCK - 1) / MP_BLOCK;
    p.count_bytes = MP_COUNT_BYTES;
    p.tile_bytes = round256(p.tiles * 16) + round256(p.tiles * 4);
    const size_t widest = p.depth ? p.in[1] : 1;
    p.list_bytes = round256(widest * sizeof(uint4));
    p.value_bytes = widest * 32;
    return p;
}

hipError_t launch_multiproof(const MultiproofPlan& p, const void* leaves, const void* levels, const void* indices, void* leaves_out,
                             void* proof, size_t proof_cap, void* proof_len, void* n_bad, void* work, hipStream_t st) {
    const MpWork w = mp_work(p, work);
    hipError_t e = mp_begin(p, w, indices, leaves, leaves_out, n_bad, st);
    for (unsigned l = 0; l < p.depth && e == hipSuccess; ++l) {
        const void* src = l == 0 ? leaves : static_cast<const void*>(static_cast<const char*>(levels) + p.start[l] * 32);
        e = p.arity == 4 ? mp_step<4, true>(p, w, l, indices, src, proof, proof_cap, st)
                         : mp_step<2, true>(p, w, l, indices, src, proof, proof_cap, st);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mp_finish_extract, dim3(1), dim3(1), 0, st, w.ctr, static_cast<u64*>(proof_len));
    return hipGetLastError();
}

hipError_t launch_multiproof_verify(const int32_t* tab, const TagArg& tag, const MultiproofPlan& p, const void* indices,
                                    const void* leaves_in, const void* proof, size_t proof_len, const void* root, void* ok, void* root_out,
                                    void* n_hashed, void* n_bad, void* work, void* values, hipStream_t st) {
    const MpWork w = mp_work(p, work);
    Scalar32* vals[2] = {static_cast<Scalar32*>(values), reinterpret_cast<Scalar32*>(static_cast<char*>(values) + p.value_bytes)};
    hipError_t e = mp_begin(p, w, indices, nullptr, nullptr, n_bad, st);
    for (unsigned l = 0; l < p.depth && e == hipSuccess; ++l) {
        e = p.arity == 4 ? mp_step<4, false>(p, w, l, indices, nullptr, nullptr, 0, st)
                         : mp_step<2, false>(p, w, l, indices, nullptr, nullptr, 0, st);
        if (e != hipSuccess) break;
        MpDigest P;
        P.list = w.list[(l + 1) & 1];
        P.count = w.ctr + (l + 1);
        P.vals_in = l == 0 ? static_cast<const Scalar32*>(leaves_in) : vals[l & 1];
        P.vals_out = vals[(l + 1) & 1];
        P.proof = static_cast<const Scalar32*>(proof);
        P.proof_len = proof_len;
        P.w_below = p.w[l];
        P.w_node = nullptr;
        e = mp_digests(tab, tag, p.arity, P, p.in[l + 1], st);
    }
    if (e != hipSuccess) return e;
    const void* top = p.depth == 0 ? leaves_in : static_cast<const void*>(vals[p.depth & 1]);
    hipLaunchKernelGGL(k_mp_finish_verify, dim3(1), dim3(1), 0, st, w.ctr, p.depth, (uint64_t)proof_len, static_cast<const uint4*>(top),
                       static_cast<const uint4*>(root), static_cast<uint8_t*>(ok), static_cast<uint4*>(root_out),
                       static_cast<u64*>(n_hashed));
    return hipGetLastError();
}

}  // namespace p252
