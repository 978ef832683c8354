// forest_update.h — launch interface between api_forest.cpp and forest_update.hip: k leaf updates (tree id, leaf id, new leaf) anywhere
// in a built forest of trees of DIFFERENT sizes (p252_merkle{4,2}_forest_ragged_update_device), every dirty node hashed once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "forest_ragged.h"
#include "kernels.h"

namespace p252 {

// The host's view of one call, all derived from (n_leaves, n_trees, max_leaves, k).  Level l (1 .. depth) has at most
// in[l] = min(k, bound[l]) dirty nodes (bound[l] = n_leaves / arity^l + n_trees: ForestRaggedPlan; in[0] = k, the updates
// themselves).  The scratch holds ids only: two lists of k 16-byte records (tree id, node index), level l - 1's and level l's, one
// uint64 counter per level, and the claim table of the widest level.
struct ForestUpdatePlan {
    unsigned arity = 4, log2a = 2, depth = 0;
    size_t n_trees = 0, k = 0;
    size_t in[FOREST_RAGGED_MAX_DEPTH + 1] = {};     // most records of level l's list
    size_t slots[FOREST_RAGGED_MAX_DEPTH + 1] = {};  // claim-table slots of level l: a power of two >= 2 in[l - 1]
    size_t list_bytes = 0, count_bytes = 0, table_bytes = 0;
    size_t ids_bytes() const { return 2 * list_bytes + count_bytes; }  // beside the forest's index, in one buffer
    // inside that buffer: the counters, then the two lists (level l's records are list l & 1)
    unsigned long long* counts(void* ids) const { return static_cast<unsigned long long*>(ids); }
    uint4* list(void* ids, unsigned l) const { return reinterpret_cast<uint4*>(static_cast<char*>(ids) + count_bytes + (l & 1) * list_bytes); }
};
ForestUpdatePlan forest_update_plan(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);

// One level's digests on a list the caller made: record g < *count of `list` (16 bytes: tree id, valid, node index low and high, as
// k_fu_claim writes them) names node i of level `level` >= 1 of tree t; it is hashed from level - 1 of the tree (its leaves for level
// 1) into the tree's block of `levels`, and into roots[t] when it is the tree's top.  bound = the host's bound of *count: it sizes
// the launch and picks the kernel.  *n_hashed (may be null, as roots) grows by *count.  ntree / lo / offsets: the forest's index.
struct ForestDigestList {
    const void* list = nullptr;
    const unsigned long long* count = nullptr;
    size_t bound = 0;
    const uint64_t* ntree = nullptr;
    const uint64_t* lo = nullptr;
    const void* offsets = nullptr;
    const void* leaves = nullptr;
    void* levels = nullptr;
    void* roots = nullptr;
    void* n_hashed = nullptr;
    unsigned level = 1;
};
hipError_t launch_forest_digest_list(const int32_t* tab, const TagArg& tag, unsigned arity, unsigned log2a, const ForestDigestList& list,
                                     hipStream_t st);

// a claim table of `slots` slots (a power of two): the shift that takes a key's 64-bit hash to its slot
inline unsigned shift_of(size_t slots) {
    unsigned shift = 64;
    for (size_t s = slots; s > 1; s >>= 1) --shift;
    return shift;
}

// what level l's claim kernel is launched with: list l - 1 (in_count null for l == 1: all `lanes` records) -> list l
struct ForestClaimLevel {
    unsigned level = 1, shift = 64;
    const uint4* in = nullptr;
    const unsigned long long* in_count = nullptr;
    size_t lanes = 0;
    unsigned long long* table = nullptr;
    uint4* out = nullptr;
    unsigned long long* out_count = nullptr;
};

// Levels 1 .. plan.depth of an update whose list 0 is written (plan.list(ids, 0)): per level the claim table is cleared to 0xFF bytes,
// enqueue_claim(ForestClaimLevel) launches the caller's claim kernel, and the level's digests follow.  `d` carries the forest (ntree,
// lo, offsets, leaves, levels, roots, n_hashed); the list, count, bound and level are filled here.
template <class EnqueueClaim>
hipError_t launch_forest_update_levels(const int32_t* tab, const TagArg& tag, const ForestUpdatePlan& p, ForestDigestList d, void* ids,
                                       void* table, hipStream_t st, EnqueueClaim enqueue_claim) {
    unsigned long long* count = p.counts(ids);
    hipError_t e = hipMemsetAsync(count, 0, p.count_bytes, st);
    if (e != hipSuccess) return e;
    for (unsigned l = 1; l <= p.depth; ++l) {
        e = hipMemsetAsync(table, 0xFF, p.slots[l] * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
        ForestClaimLevel c;
        c.level = l;
        c.shift = shift_of(p.slots[l]);
        c.in = p.list(ids, l - 1);
        c.in_count = l == 1 ? nullptr : count + (l - 1);
        c.lanes = p.in[l - 1];
        c.table = static_cast<unsigned long long*>(table);
        c.out = p.list(ids, l);
        c.out_count = count + l;
        enqueue_claim(c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        d.list = c.out;
        d.count = c.out_count;
        d.bound = p.in[l];
        d.level = l;
        e = launch_forest_digest_list(tab, tag, p.arity, p.log2a, d, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The whole update on `st`: ntree / lo = the forest's index (launch_forest_ragged_index); ids = plan.ids_bytes() and table =
// plan.table_bytes of scratch.  roots, n_bad (uint32), n_hashed (uint64) may be null; levels may be null when plan.depth == 0.
hipError_t launch_forest_update(const int32_t* tab, const TagArg& tag, const ForestUpdatePlan& plan, void* leaves, const void* offsets,
                                const uint64_t* ntree, const uint64_t* lo, void* levels, const void* tree_ids, const void* leaf_ids,
                                const void* new_leaves, void* roots, void* n_bad, void* n_hashed, void* ids, void* table, hipStream_t st);

}  // namespace p252
