// forest_journal.hip — the leaf update of forest_update.hip with a journal, and the swap that plays the journal back: every leaf
// and every node the update overwrites is first saved as (id, old 32 bytes), so that leaving the update again, and entering it
// again after that, is an exchange of bytes at memory speed with no digest at all.
//   k_fj_leaves    one lane per update, validated as k_fu_scatter validates it (forest_tree_leaves).  The leaf's slot in d_leaves
//                  (offsets[t] + leaf, unique across the forest) is claimed in an open-addressing table with one 64-bit
//                  compare-and-swap, as k_fu_claim claims a node: of a pair given several times ONE lane wins and stores its whole
//                  scalar, so the value that lands is never a mix and the old value is read by one lane only.  The winner appends
//                  a journal entry with the old leaf (one atomic add per wave: ballot, popcount, the leader's base broadcast),
//                  then stores the new leaf, its record of list 0 and the root of a one-leaf tree.  Losers and bad updates write
//                  a void record.
//   k_fj_claim     k_fu_claim's work for level l = 1 .. D; the lane that installs the parent's key also reads the parent's old
//                  32 bytes — the key IS its slot in d_levels — and appends them to the journal before the level's digests run.
//   k_fj_swap      one lane per journal entry: the id is checked against the forest's index, then the entry's 32 bytes and the
//                  node's change places; an entry that is its tree's top rewrites the root as well.
// The level digests are forest_update.hip's (launch_forest_digest_list), and the address arithmetic is forest_node.hpp's.
// A journal entry is written by the lane that won the claim of its node, so the entries of one call name distinct nodes: the
// swap's lanes touch disjoint bytes of the forest and disjoint bytes of the journal.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "blockops.hpp"
#include "forest_journal.h"
#include "forest_node.hpp"
#include "forest_update.h"
#include "kernels.h"

namespace p252 {

namespace {

constexpr unsigned FJ_BLOCK = 256;

// a journal id: level 0 = the leaves
__device__ __forceinline__ uint4 journal_id(uint32_t t, unsigned level, uint64_t i) {
    return make_uint4(t, level + 1u, (unsigned)i, (unsigned)(i >> 32));
}

struct Journal {
    uint4* ids;
    uint4* values;
    unsigned long long cap;
    unsigned long long* len;
};

// (the host refused a capacity below the call's bound, so at < cap; the test keeps a journal that is too short from being overrun)
__device__ __forceinline__ void journal_put(const Journal& J, unsigned long long at, uint4 id, uint4 lo, uint4 hi) {
    if (at >= J.cap) return;
    J.ids[at] = id;
    J.values[2 * at] = lo;
    J.values[2 * at + 1] = hi;
}

}  // namespace

// ---- the leaves, list 0 and the journal's level-0 entries ----
__global__ void __launch_bounds__(FJ_BLOCK) k_fj_leaves(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                        size_t n_trees, const uint32_t* __restrict__ tree_ids,
                                                        const uint64_t* __restrict__ leaf_ids, const uint4* __restrict__ new_leaves, size_t k,
                                                        uint4* __restrict__ leaves, uint4* __restrict__ roots, uint4* __restrict__ list,
                                                        unsigned* __restrict__ n_bad, unsigned long long* __restrict__ table, unsigned shift,
                                                        Journal J) {
    const size_t i = (size_t)blockIdx.x * FJ_BLOCK + threadIdx.x;
    // (no early return: the whole wave takes part in the append below)
    const bool live = i < k;
    const uint32_t t = live ? tree_ids[i] : 0u;
    const uint64_t leaf = live ? leaf_ids[i] : 0ull;
    size_t ts;
    const uint64_t n = forest_tree_leaves(ntree, n_trees, t, &ts);
    const bool good = live && n != 0 && leaf < n;
    if (live && !good && n_bad) atomicAdd(n_bad, 1u);  // a bad update: nothing written, no record
    const size_t at = good ? 2 * (size_t)(offsets[ts] + leaf) : 0;  // (inside the tree: k_fr_prep checked offsets[t + 1] <= n_leaves)
    const bool won = good && claim(table, shift, (unsigned long long)(at >> 1));
    if (live && !won) list[i] = make_uint4(0u, 0u, 0u, 0u);
    const unsigned long long winners = __ballot(won);
    if (winners == 0) return;
    const unsigned long long place = append_place(won, winners, J.len);
    if (!won) return;
    journal_put(J, place, journal_id(t, 0u, leaf), leaves[at], leaves[at + 1]);
    leaves[at] = new_leaves[2 * i];
    leaves[at + 1] = new_leaves[2 * i + 1];
    if (n == 1 && roots)  // (the leaf keeps its bytes; the root is reduced, as every output and as the forest's build writes it)
        store_scalar(reinterpret_cast<Scalar32*>(roots) + ts, load_scalar(reinterpret_cast<const Scalar32*>(new_leaves) + i));
    list[i] = record(t, leaf);
}

// ---- level l's distinct dirty nodes: list l - 1 -> list l, and their old values -> the journal ----
__global__ void __launch_bounds__(FJ_BLOCK) k_fj_claim(const uint4* __restrict__ in, const unsigned long long* __restrict__ in_count,
                                                       size_t lanes, const uint64_t* __restrict__ ntree, const uint64_t* __restrict__ LO,
                                                       unsigned l, unsigned la, unsigned long long* __restrict__ table, unsigned shift,
                                                       uint4* __restrict__ out, unsigned long long* __restrict__ out_count,
                                                       const uint4* __restrict__ levels, Journal J) {
    const size_t g = (size_t)blockIdx.x * FJ_BLOCK + threadIdx.x;
    bool live = g < lanes && (!in_count || g < *in_count);
    const uint4 r = live ? in[g] : make_uint4(0u, 0u, 0u, 0u);
    live = live && r.y != 0;
    const uint32_t t = r.x;
    const uint64_t n = live ? ntree[t] : 0ull;
    live = live && ceil_shift(n, (l - 1) * la) > 1;  // level l - 1 has more than one node: the tree has a level l
    const uint64_t parent = u64_of(r.z, r.w) >> la;
    const unsigned long long slot = live ? LO[t] + level_start(n, l, la) + parent : 0ull;  // where fu_node's `out` points
    const bool won = live && claim(table, shift, slot);
    const unsigned long long winners = __ballot(won);
    if (winners == 0) return;
    const unsigned long long place = append_place(won, winners, out_count);
    const unsigned long long jplace = append_place(won, winners, J.len);
    if (!won) return;
    out[place] = record(t, parent);
    journal_put(J, jplace, journal_id(t, l, parent), levels[2 * slot], levels[2 * slot + 1]);
}

// ---- the journal played back: entry <-> node ----
__global__ void __launch_bounds__(FJ_BLOCK) k_fj_swap(Journal J, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntree,
                                                      const uint64_t* __restrict__ LO, size_t n_trees, unsigned la, uint4* leaves,
                                                      uint4* levels, uint4* roots, unsigned* n_bad) {
    const unsigned long long g = (unsigned long long)blockIdx.x * FJ_BLOCK + threadIdx.x;
    if (g >= J.cap || g >= *J.len) return;
    const uint4 id = J.ids[g];
    size_t ts;
    const uint64_t n = forest_tree_leaves(ntree, n_trees, id.x, &ts);  // 0: an unknown or a bad tree
    const uint64_t i = u64_of(id.z, id.w);
    const unsigned level = id.y - 1u;
    // nodes of the named level: 0 for a void id (id.y == 0) and for a level above the tree's top
    uint64_t nodes = 0;
    if (id.y != 0 && level <= FOREST_RAGGED_MAX_DEPTH) nodes = level == 0 ? n : level_nodes(n, level, la);
    if (i >= nodes) {  // names no node of this forest: nothing written
        if (n_bad) atomicAdd(n_bad, 1u);
        return;
    }
    uint4* node = level == 0 ? leaves + 2 * (size_t)(offsets[ts] + i) : levels + 2 * (size_t)(LO[ts] + level_start(n, level, la) + i);
    const uint4 jlo = J.values[2 * g], jhi = J.values[2 * g + 1];
    const uint4 flo = node[0], fhi = node[1];
    node[0] = jlo;
    node[1] = jhi;
    if (roots && nodes == 1) {  // the tree's top stands for its root
        if (level == 0)         // (a one-leaf tree: the leaf keeps its bytes, the root is reduced, as k_fj_leaves writes it)
            store_scalar(reinterpret_cast<Scalar32*>(roots) + ts, load_scalar(reinterpret_cast<const Scalar32*>(J.values) + g));
        else {
            roots[2 * ts] = jlo;
            roots[2 * ts + 1] = jhi;
        }
    }
    J.values[2 * g] = flo;
    J.values[2 * g + 1] = fhi;
}

// ---------------------------------------------------------------------------------------------
// launchers (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
size_t forest_journal_bound(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k) {
    if (n_leaves == 0 || n_trees == 0 || max_leaves == 0 || k == 0) return 0;
    const unsigned la = arity == 4 ? 2 : 1;
    const unsigned depth = forest_ragged_depth(max_leaves < n_leaves ? max_leaves : n_leaves, arity);
    size_t total = k;
    for (unsigned l = 1; l <= depth; ++l) {
        const size_t wide = l * la < 64 ? n_leaves >> (l * la) : 0;
        const size_t bound = wide > SIZE_MAX - n_trees ? SIZE_MAX : wide + n_trees;  // ForestRaggedPlan::bound[l]
        const size_t in = k < bound ? k : bound;
        if (in > SIZE_MAX - total) return SIZE_MAX;
        total += in;
    }
    return total;
}

ForestJournalPlan forest_journal_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k) {
    ForestJournalPlan p;
    p.up = forest_update_plan(arity, n_leaves, n_trees, max_leaves, k);
    p.slots0 = CLAIM_MIN_SLOTS;
    while (p.slots0 < 2 * k) p.slots0 <<= 1;
    const size_t bytes0 = p.slots0 * sizeof(unsigned long long);
    p.table_bytes = bytes0 > p.up.table_bytes ? bytes0 : p.up.table_bytes;
    p.bound = forest_journal_bound(arity, n_leaves, n_trees, max_leaves, k);
    return p;
}

hipError_t launch_forest_update_journaled(const int32_t* tab, const TagArg& tag, const ForestJournalPlan& plan, void* leaves,
                                          const void* offsets, const uint64_t* ntree, const uint64_t* lo, void* levels, const void* tree_ids,
                                          const void* leaf_ids, const void* new_leaves, void* roots, void* n_bad, void* n_hashed,
                                          const ForestJournal& j, void* ids, void* table, hipStream_t st) {
    const ForestUpdatePlan& p = plan.up;
    if (p.k == 0) return hipSuccess;
    unsigned long long* tb = static_cast<unsigned long long*>(table);
    const uint64_t* off = static_cast<const uint64_t*>(offsets);
    const Journal J{static_cast<uint4*>(j.ids), static_cast<uint4*>(j.values), (unsigned long long)j.cap,
                    static_cast<unsigned long long*>(j.len)};
    hipError_t e = hipMemsetAsync(j.len, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(tb, 0xFF, plan.slots0 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fj_leaves, dim3((unsigned)((p.k + FJ_BLOCK - 1) / FJ_BLOCK)), dim3(FJ_BLOCK), 0, st, off, ntree, p.n_trees,
                       static_cast<const uint32_t*>(tree_ids), static_cast<const uint64_t*>(leaf_ids), static_cast<const uint4*>(new_leaves),
                       p.k, static_cast<uint4*>(leaves), static_cast<uint4*>(roots), p.list(ids, 0), static_cast<unsigned*>(n_bad), tb,
                       shift_of(plan.slots0), J);
    e = hipGetLastError();
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
        hipLaunchKernelGGL(k_fj_claim, dim3((unsigned)((c.lanes + FJ_BLOCK - 1) / FJ_BLOCK)), dim3(FJ_BLOCK), 0, st, c.in, c.in_count, c.lanes,
                           ntree, lo, c.level, p.log2a, c.table, c.shift, c.out, c.out_count, static_cast<const uint4*>(levels), J);
    });
}

hipError_t launch_forest_journal_swap(unsigned arity, void* leaves, const void* offsets, const uint64_t* ntree, const uint64_t* lo,
                                      size_t n_trees, void* levels, const ForestJournal& j, void* roots, void* n_bad, hipStream_t st) {
    if (j.cap == 0) return hipSuccess;
    const Journal J{static_cast<uint4*>(j.ids), static_cast<uint4*>(j.values), (unsigned long long)j.cap,
                    static_cast<unsigned long long*>(j.len)};
    hipLaunchKernelGGL(k_fj_swap, dim3((unsigned)((j.cap + FJ_BLOCK - 1) / FJ_BLOCK)), dim3(FJ_BLOCK), 0, st, J,
                       static_cast<const uint64_t*>(offsets), ntree, lo, n_trees, arity == 4 ? 2u : 1u, static_cast<uint4*>(leaves),
                       static_cast<uint4*>(levels), static_cast<uint4*>(roots), static_cast<unsigned*>(n_bad));
    return hipGetLastError();
}

}  // namespace p252
