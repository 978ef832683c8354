// api_forest.cpp — the ragged-forest family of the C ABI (include/poseidon252_hip.h): every entry point whose name holds
// _forest_ragged_, _path_ragged_, _forest_frontier_, _forest_consistency_ or _forest_range_, with the checks they share.  Host side only, as api.cpp:
// argument rules and launch sequencing; the kernels are in the forest_*.hip files.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/poseidon252_hip.h"
#include "api_util.hpp"
#include "ctx.hpp"
#include "forest_anchor.h"
#include "forest_append.h"
#include "forest_consistency.h"
#include "forest_frontier.h"
#include "forest_journal.h"
#include "forest_multiproof.h"
#include "forest_openings.h"
#include "forest_ragged.h"
#include "forest_range.h"
#include "forest_sequential.h"
#include "forest_update.h"
#include "forest_witness.h"
#include "kernels.h"
#include "pairs.h"
#include "ragged.h"

using namespace p252;
using namespace p252host;

namespace {
// with_stream_scratch for the calls that start from the index of a ragged forest (forest_ragged.h): the index takes the head of the
// first buffer, `extra0` bytes follow it, and body(ntree, lo, rest0, buf1) enqueues the call's own launches behind the index's
template <class Body>
int with_forest_index(p252_ctx* ctx, const char* who, hipStream_t st, unsigned arity, const void* d_offsets, size_t n_trees,
                      size_t n_leaves, size_t max_leaves, size_t extra0, size_t need1, Body&& body) {
    const size_t index_bytes = forest_ragged_index_bytes(n_trees);
    return with_stream_scratch(ctx, who, st, index_bytes + extra0, need1, [&](p252_ctx::LevelSet& set) {
        char* meta = static_cast<char*>(set.buf[0]);
        const uint64_t *ntree = nullptr, *lo = nullptr;
        const hipError_t e = launch_forest_ragged_index(arity, d_offsets, n_trees, n_leaves, max_leaves, meta, &ntree, &lo, st);
        if (e != hipSuccess) return e;
        return body(ntree, lo, meta + index_bytes, set.buf[1]);
    });
}

// (ByteRange / refuse_overlaps, the refusal of overlapping buffers: api_util.hpp)

// the bound on the stored levels of a ragged forest, in scalars: what d_levels of these sizes holds
size_t forest_levels_bound(unsigned arity, size_t n_leaves, size_t n_trees, size_t max_leaves) {
    return n_leaves / (arity - 1) + n_trees * forest_ragged_depth(max_leaves, arity);
}
}  // namespace

extern "C" {

// ---- a forest of trees of different sizes in one call (forest_ragged.hip): the bookkeeping (leaf counts, scans, first tree of
// each block) and, without d_levels, the level-major ping-pong live in the scratch pair of the calling stream
// every forest call's sizes: the bookkeeping inside size_t; the good trees' leaf counts, summed on the device, below 2^63.  k: the callers'.
static int forest_shape_check(const Refusal& refuse, size_t n_leaves, size_t n_trees, size_t max_leaves) {
    const size_t eff_max = max_leaves < n_leaves ? max_leaves : n_leaves;
    if (n_leaves > SIZE_MAX / 64 || n_trees > SIZE_MAX / 8 / (FOREST_RAGGED_MAX_DEPTH + 2) || (eff_max && n_trees > (SIZE_MAX / 2) / eff_max))
        return refuse("size overflow");
    return P252_OK;
}

static int forest_ragged_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_roots, void* d_levels, void* d_n_bad,
                                void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_forest_ragged"};
    if (n_trees == 0) return P252_OK;
    if (max_leaves == 0) return refuse("max_leaves must be > 0");
    if (!tag || !d_leaves || !d_offsets || !d_roots) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_roots, d_levels})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestRaggedPlan plan = forest_ragged_plan(arity, n_leaves, n_trees, max_leaves, d_levels != nullptr);
    const bool ping = !d_levels && plan.depth > 0;
    return with_stream_scratch(ctx, refuse.who, st, plan.meta_bytes + (ping ? plan.bound[1] * 32 : 0),
                               ping && plan.depth > 1 ? plan.bound[2] * 32 : 0, [&](p252_ctx::LevelSet& set) {
                                   char* meta = static_cast<char*>(set.buf[0]);
                                   return launch_forest_ragged(ctx->d_tab, tag_arg(tag), plan, d_leaves, d_offsets, max_leaves, d_roots, d_levels,
                                                               d_n_bad, meta, ping ? meta + plan.meta_bytes : nullptr, set.buf[1], st);
                               });
}

P252_MERKLE_PAIR(int, forest_ragged_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                  size_t max_leaves, void* d_roots, void* d_levels, void* d_n_bad, void* hip_stream),
                 forest_ragged_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_roots, d_levels, d_n_bad, hip_stream))

// ---- openings out of such a forest, their re-hash with a depth per opening, and a root per opening (forest_openings.hip).  The
// scratch — the forest's index and the opening records; the sort's order and counters; the recomputed roots — is the pair of the
// calling stream, as for the build ----
static int forest_ragged_openings_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                         size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                         const void* d_leaf_ids, size_t k, void* d_leaves_out, void* d_siblings, void* d_positions,
                                         void* d_depths, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_ragged_openings"};
    if (int rc = refuse.unless_built_forest(n_leaves, n_trees, max_leaves)) return rc;
    const size_t depth = forest_ragged_depth(max_leaves, arity);
    if (!d_leaves || !d_offsets || !d_tree_ids || !d_leaf_ids || !d_leaves_out || !d_depths ||
        (depth && (!d_levels || !d_siblings || !d_positions)))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_siblings})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_leaf_ids)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    if (k > SIZE_MAX / 128 / (depth ? depth : 1)) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, forest_openings_record_bytes(k), 0,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* records, void*) {
                                 return launch_forest_openings(arity, d_leaves, d_levels, d_offsets, ntree, lo, n_trees, d_tree_ids, d_leaf_ids, k,
                                                               (unsigned)depth, records, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad, st);
                             });
}

// the argument checks of the re-hash (shared with the verify call)
static int path_ragged_check(const Refusal& refuse, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                             const void* d_positions, const void* d_depths, size_t stride_depth, size_t k) {
    if (stride_depth > FOREST_OPENINGS_MAX_DEPTH) return refuse("stride_depth must be <= 64");
    if (!tag || !d_leaves_in || !d_depths || (stride_depth && (!d_siblings || !d_positions))) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves_in, stride_depth ? d_siblings : nullptr})) return rc;
    if (k > SIZE_MAX / 128 / (stride_depth ? stride_depth : 1)) return refuse("size overflow");
    return P252_OK;
}

static int path_ragged_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                              const void* d_positions, const void* d_depths, size_t stride_depth, void* d_roots_out, size_t k,
                              void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_path_ragged"};
    if (int rc = path_ragged_check(refuse, tag, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, k)) return rc;
    if (!d_roots_out) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_roots_out})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!ragged_sort_enabled()) {  // P252_RAGGED_SORT=0: identity order, no scratch
        HIP_TRY(ctx, launch_path_ragged(arity, ctx->d_tab, tag_arg(tag), d_leaves_in, d_siblings, d_positions, d_depths, (unsigned)stride_depth,
                                        d_roots_out, k, d_n_bad, nullptr, nullptr, st));
        return P252_OK;
    }
    return with_stream_scratch(ctx, refuse.who, st, forest_openings_order_bytes(k), forest_openings_hist_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_path_ragged(arity, ctx->d_tab, tag_arg(tag), d_leaves_in, d_siblings, d_positions, d_depths, (unsigned)stride_depth,
                                  d_roots_out, k, d_n_bad, set.buf[0], set.buf[1], st);
    });
}

static int forest_ragged_verify_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                                       const void* d_positions, const void* d_depths, size_t stride_depth, const void* d_tree_ids,
                                       const void* d_roots, size_t n_trees, void* d_ok, size_t k, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_ragged_verify"};
    if (int rc = path_ragged_check(refuse, tag, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, k)) return rc;
    if (!d_tree_ids || !d_ok || (n_trees && !d_roots)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_roots})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids)})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool sort = ragged_sort_enabled();
    // the recomputed roots (k x 32 bytes), then the sort's order; the counters in the second buffer
    return with_stream_scratch(ctx, refuse.who, st, k * 32 + (sort ? forest_openings_order_bytes(k) : 0), sort ? forest_openings_hist_bytes() : 0,
                               [&](p252_ctx::LevelSet& set) {
                                   char* roots = static_cast<char*>(set.buf[0]);
                                   const hipError_t e = launch_path_ragged(arity, ctx->d_tab, tag_arg(tag), d_leaves_in, d_siblings, d_positions, d_depths,
                                                                           (unsigned)stride_depth, roots, k, nullptr, sort ? roots + k * 32 : nullptr,
                                                                           sort ? set.buf[1] : nullptr, st);
                                   if (e != hipSuccess) return e;
                                   return launch_compare_roots_gather(roots, d_depths, (unsigned)stride_depth, d_tree_ids, d_roots, n_trees, d_ok, k, st);
                               });
}

P252_MERKLE_PAIR(int, forest_ragged_openings_device,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_leaves_out, void* d_siblings,
                  void* d_positions, void* d_depths, void* d_n_bad, void* hip_stream),
                 forest_ragged_openings_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k,
                                               d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad, hip_stream))

P252_MERKLE_PAIR(int, path_ragged_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings, const void* d_positions,
                  const void* d_depths, size_t stride_depth, void* d_roots_out, size_t k, void* d_n_bad, void* hip_stream),
                 path_ragged_device(ctx, arity, tag, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, d_roots_out, k, d_n_bad, hip_stream))

P252_MERKLE_PAIR(int, forest_ragged_verify_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings, const void* d_positions,
                  const void* d_depths, size_t stride_depth, const void* d_tree_ids, const void* d_roots, size_t n_trees, void* d_ok, size_t k,
                  void* hip_stream),
                 forest_ragged_verify_device(ctx, arity, tag, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, d_tree_ids, d_roots,
                                             n_trees, d_ok, k, hip_stream))

// what the journaled update and the journal's swap (both further down) ask of the journal's three buffers
static int journal_check(const Refusal& refuse, const void* d_journal_ids, const void* d_journal_values, size_t journal_cap,
                         const void* d_journal_len) {
    if (!d_journal_len || (journal_cap && (!d_journal_ids || !d_journal_values))) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_journal_ids, d_journal_values})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_journal_len)})) return rc;
    if (journal_cap > SIZE_MAX / 64) return refuse("size overflow");
    return P252_OK;
}

// ---- leaf updates anywhere in such a forest in one call, every dirty node hashed once (forest_update.hip).  The scratch — the
// forest's index, two lists of node ids and the per-level counters; the claim table in the second buffer — is the pair of the
// calling stream; it holds ids only, never a copy of the new leaves ----
// `j`: the journaled update (forest_journal.hip), which asks its own checks of the journal first and of its capacity last
static int forest_ragged_update_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                       const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels, const void* d_tree_ids,
                                       const void* d_leaf_ids, const void* d_new_leaves, size_t k, void* d_roots, void* d_n_bad,
                                       void* d_n_hashed, const ForestJournal* j, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, j ? "merkle_forest_ragged_update_journaled" : "merkle_forest_ragged_update"};
    hipStream_t st = (hipStream_t)hip_stream;
    if (j) {
        if (int rc = journal_check(refuse, j->ids, j->values, j->cap, j->len)) return rc;
        if (k == 0) {  // no update, an empty journal: the length is the one thing the call always sets
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipMemsetAsync(j->len, 0, 8, st));
        }
    }
    if (k == 0) return P252_OK;
    if (int rc = refuse.unless_built_forest(n_leaves, n_trees, max_leaves)) return rc;
    const size_t depth = forest_ragged_depth(max_leaves < n_leaves ? max_leaves : n_leaves, arity);
    if (!tag || !d_leaves || !d_offsets || !d_tree_ids || !d_leaf_ids || !d_new_leaves || (depth && !d_levels)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_new_leaves, d_roots})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_leaf_ids), P252_NAMED(d_n_hashed)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    if (k > SIZE_MAX / 128) return refuse("size overflow");
    const ForestJournalPlan plan = forest_journal_plan(arity, n_leaves, n_trees, max_leaves, k);  // (plan.up: the plain update's)
    if (j && j->cap < plan.bound)  // (nothing is enqueued: the device can never run past the journal)
        return refuse("journal_cap " + std::to_string(j->cap) + " is below the call's bound of " + std::to_string(plan.bound) + " entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t table_bytes = j ? plan.table_bytes : plan.up.table_bytes;  // (the journal's claim table also serves level 0)
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, plan.up.ids_bytes(), table_bytes,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* ids, void* table) {
                                 if (j)
                                     return launch_forest_update_journaled(ctx->d_tab, tag_arg(tag), plan, d_leaves, d_offsets, ntree, lo, d_levels,
                                                                           d_tree_ids, d_leaf_ids, d_new_leaves, d_roots, d_n_bad, d_n_hashed, *j, ids,
                                                                           table, st);
                                 return launch_forest_update(ctx->d_tab, tag_arg(tag), plan.up, d_leaves, d_offsets, ntree, lo, d_levels, d_tree_ids,
                                                             d_leaf_ids, d_new_leaves, d_roots, d_n_bad, d_n_hashed, ids, table, st);
                             });
}

P252_MERKLE_PAIR(int, forest_ragged_update_device,
                 (p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  void* d_levels, const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, size_t k, void* d_roots, void* d_n_bad,
                  void* d_n_hashed, void* hip_stream),
                 forest_ragged_update_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                             d_new_leaves, k, d_roots, d_n_bad, d_n_hashed, nullptr, hip_stream))

// ---- the same update with a journal of every leaf and node it overwrites, and the swap that plays the journal back: undo, then
// redo, with no digest (forest_journal.hip).  The update's scratch is the plain update's, its claim table also serving level 0; the
// swap's is the forest's index alone.  The journal is the caller's ----
P252_MERKLE_PAIR(size_t, forest_ragged_journal_bound, (size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k),
                 forest_journal_bound(arity, n_leaves, n_trees, max_leaves, k))

static int forest_ragged_update_journaled_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                       const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                       const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, size_t k,
                                                       void* d_roots, void* d_n_bad, void* d_n_hashed, void* d_journal_ids,
                                                       void* d_journal_values, size_t journal_cap, void* d_journal_len, void* hip_stream) {
    const ForestJournal j{d_journal_ids, d_journal_values, journal_cap, d_journal_len};
    return forest_ragged_update_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                       d_new_leaves, k, d_roots, d_n_bad, d_n_hashed, &j, hip_stream);
}

P252_MERKLE_PAIR(int, forest_ragged_update_journaled_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  void* d_levels, const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, size_t k, void* d_roots, void* d_n_bad,
                  void* d_n_hashed, void* d_journal_ids, void* d_journal_values, size_t journal_cap, void* d_journal_len, void* hip_stream),
                 forest_ragged_update_journaled_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids,
                                                       d_leaf_ids, d_new_leaves, k, d_roots, d_n_bad, d_n_hashed, d_journal_ids, d_journal_values,
                                                       journal_cap, d_journal_len, hip_stream))

static int forest_ragged_journal_swap_device(p252_ctx* ctx, unsigned arity, void* d_leaves, size_t n_leaves, const void* d_offsets,
                                             size_t n_trees, size_t max_leaves, void* d_levels, void* d_journal_ids, void* d_journal_values,
                                             size_t journal_cap, const void* d_journal_len, void* d_roots, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (journal_cap == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_ragged_journal_swap"};
    if (int rc = journal_check(refuse, d_journal_ids, d_journal_values, journal_cap, d_journal_len)) return rc;
    if (int rc = refuse.unless_built_forest(n_leaves, n_trees, max_leaves)) return rc;
    const size_t depth = forest_ragged_depth(max_leaves < n_leaves ? max_leaves : n_leaves, arity);
    if (!d_leaves || !d_offsets || (depth && !d_levels)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_roots})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestJournal j{d_journal_ids, d_journal_values, journal_cap, const_cast<void*>(d_journal_len)};  // (read only: k_fj_swap never writes the length)
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, 0, 0,
                             [&](const uint64_t* ntree, const uint64_t* lo, char*, void*) {
                                 return launch_forest_journal_swap(arity, d_leaves, d_offsets, ntree, lo, n_trees, d_levels, j, d_roots, d_n_bad, st);
                             });
}

P252_MERKLE_PAIR(int, forest_ragged_journal_swap_device_into,
                 (p252_ctx* ctx, void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                  void* d_journal_ids, void* d_journal_values, size_t journal_cap, const void* d_journal_len, void* d_roots, void* d_n_bad,
                  void* hip_stream),
                 forest_ragged_journal_swap_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_journal_ids,
                                                   d_journal_values, journal_cap, d_journal_len, d_roots, d_n_bad, hip_stream))

// ---- leaves appended to the trees of such a forest, written as a new compact forest: clean nodes moved, dirty ones hashed once
// (forest_append.hip).  The scratch — the indices of both forests, two words per tree, one scan row per level, the first-tree rows of
// the relocation tiles; the dirty lists in the second buffer — is the pair of the calling stream; it holds ids and counts only ----
// resize: the call that also cuts (d_keep, NULL = every tree whole) and may drop trailing trees; the append is its d_keep == NULL,
// n_trees_new >= n_trees case, under its own name in the messages
static int forest_ragged_append_device_into(p252_ctx* ctx, bool resize, unsigned arity, const uint64_t tag[4], const void* d_leaves,
                                            size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                            const void* d_keep, const void* d_add, size_t n_add, const void* d_add_offsets, size_t n_trees_new,
                                            size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new,
                                            void* d_levels_new, size_t levels_cap, void* d_roots, void* d_n_bad, void* d_n_hashed,
                                            void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (n_trees_new == 0) return P252_OK;
    const Refusal refuse{ctx, resize ? "merkle_forest_ragged_resize" : "merkle_forest_ragged_append"};
    if (max_leaves_new == 0 || max_leaves_new < max_leaves) return refuse("max_leaves_new must be > 0 and >= max_leaves");
    if (!resize && n_trees_new < n_trees) return refuse("n_trees_new must be >= n_trees");
    if (n_trees && max_leaves == 0) return refuse("max_leaves must be > 0");
    if (n_leaves > SIZE_MAX / 64 || n_add > SIZE_MAX / 64) return refuse("size overflow");
    const size_t total = n_leaves + n_add;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits, both forests)
    if (int rc = forest_shape_check(refuse, total, n_trees_new, max_leaves_new)) return rc;
    if (leaves_cap > SIZE_MAX / 64 || levels_cap > SIZE_MAX / 64) return refuse("size overflow");
    if (leaves_cap < total) return refuse("leaves_cap must be >= n_leaves + n_add");
    const size_t levels_old = forest_levels_bound(arity, n_leaves, n_trees, max_leaves);
    if (levels_cap < forest_levels_bound(arity, total, n_trees_new, max_leaves_new))
        return refuse("levels_cap must be >= (n_leaves + n_add) / (arity - 1) + n_trees_new * depth(max_leaves_new)");
    if (!tag || !d_add_offsets || !d_offsets_new || !d_roots || (total && !d_leaves_new) || (n_add && !d_add) ||
        (n_trees && (!d_leaves || !d_offsets)) || (n_trees && max_leaves > 1 && !d_levels) || (max_leaves_new > 1 && !d_levels_new))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_add, d_leaves_new, d_levels_new, d_roots})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_add_offsets), P252_NAMED(d_offsets_new), P252_NAMED(d_n_hashed)}))
        return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_keep)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    const ByteRange in[] = {{d_leaves, n_trees ? n_leaves * 32 : 0, "d_leaves"},
                            {d_offsets, n_trees ? (n_trees + 1) * 8 : 0, "d_offsets"},
                            {d_levels, n_trees ? levels_old * 32 : 0, "d_levels"},
                            {d_add, n_add * 32, "d_add"},
                            {d_add_offsets, (n_trees_new + 1) * 8, "d_add_offsets"},
                            {d_keep, n_trees_new * 8, "d_keep"}};
    const ByteRange out[] = {{d_leaves_new, leaves_cap * 32, "d_leaves_new"}, {d_offsets_new, (n_trees_new + 1) * 8, "d_offsets_new"},
                             {d_levels_new, levels_cap * 32, "d_levels_new"}, {d_roots, n_trees_new * 32, "d_roots"},
                             {d_n_bad, 4, "d_n_bad"},                         {d_n_hashed, 8, "d_n_hashed"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), false)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestAppendPlan plan = forest_append_plan(arity, n_leaves, n_trees, max_leaves, n_add, n_trees_new, max_leaves_new, leaves_cap);
    return with_stream_scratch(ctx, refuse.who, st, plan.meta_bytes(), plan.list_bytes, [&](p252_ctx::LevelSet& set) {
        return launch_forest_append(ctx->d_tab, tag_arg(tag), plan, d_leaves, d_offsets, d_levels, d_keep, d_add, d_add_offsets, d_leaves_new,
                                    d_offsets_new, d_levels_new, d_roots, d_n_bad, d_n_hashed, set.buf[0], set.buf[1], st);
    });
}

P252_MERKLE_PAIR(int, forest_ragged_append_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                  size_t max_leaves, const void* d_levels, const void* d_add, size_t n_add, const void* d_add_offsets, size_t n_trees_new,
                  size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new, void* d_levels_new, size_t levels_cap,
                  void* d_roots, void* d_n_bad, void* d_n_hashed, void* hip_stream),
                 forest_ragged_append_device_into(ctx, false, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, nullptr,
                                                  d_add, n_add, d_add_offsets, n_trees_new, max_leaves_new, d_leaves_new, leaves_cap, d_offsets_new,
                                                  d_levels_new, levels_cap, d_roots, d_n_bad, d_n_hashed, hip_stream))

// ---- the same forest with each tree cut to its first k_t leaves before the append, and with trailing trees dropped: a rollback,
// a reorg, a prune.  One launcher (forest_append.hip); there is no host-buffer twin ----
P252_MERKLE_PAIR(int, forest_ragged_resize_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                  size_t max_leaves, const void* d_levels, const void* d_keep, const void* d_add, size_t n_add, const void* d_add_offsets,
                  size_t n_trees_new, size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new, void* d_levels_new,
                  size_t levels_cap, void* d_roots, void* d_n_bad, void* d_n_hashed, void* hip_stream),
                 forest_ragged_append_device_into(ctx, true, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add,
                                                  n_add, d_add_offsets, n_trees_new, max_leaves_new, d_leaves_new, leaves_cap, d_offsets_new,
                                                  d_levels_new, levels_cap, d_roots, d_n_bad, d_n_hashed, hip_stream))

// ---- any trees of one or two built forests gathered into a new compact forest (the select of forest_ragged.hip): a prune in the
// middle, a merge, a split, a reorder.  Nothing is hashed, so there is no tag.  The scratch — the indices of A, B and the new forest,
// one count per pick, the first-tree rows of the relocation tiles — is the pair of the calling stream; there is no host-buffer twin ----
static int forest_ragged_select_device_into(p252_ctx* ctx, unsigned arity, const void* d_leaves_a, size_t n_leaves_a, const void* d_offsets_a,
                                            size_t n_trees_a, size_t max_leaves_a, const void* d_levels_a, const void* d_roots_a,
                                            const void* d_leaves_b, size_t n_leaves_b, const void* d_offsets_b, size_t n_trees_b,
                                            size_t max_leaves_b, const void* d_levels_b, const void* d_roots_b, const void* d_pick,
                                            size_t n_pick, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new, void* d_levels_new,
                                            size_t levels_cap, void* d_roots_new, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_forest_ragged_select"};
    if (n_trees_a == 0) return refuse("n_trees_a must be > 0");
    if (n_pick == 0) return P252_OK;
    if (n_trees_b == 0) {  // B absent: nothing of it is read
        d_leaves_b = d_offsets_b = d_levels_b = d_roots_b = nullptr;
        n_leaves_b = max_leaves_b = 0;
    }
    if (n_leaves_a == 0 || max_leaves_a == 0) return refuse("n_leaves_a and max_leaves_a must be > 0");
    if (n_trees_b && (n_leaves_b == 0 || max_leaves_b == 0)) return refuse("n_leaves_b and max_leaves_b must be > 0");
    if (leaves_cap == 0) return refuse("leaves_cap must be > 0");
    const size_t max_leaves = max_leaves_a > max_leaves_b ? max_leaves_a : max_leaves_b;
    if (int rc = forest_shape_check(refuse, n_leaves_a, n_trees_a, max_leaves_a)) return rc;  // (the build's own limits, all three)
    if (int rc = forest_shape_check(refuse, n_leaves_b, n_trees_b, max_leaves_b)) return rc;
    if (int rc = forest_shape_check(refuse, leaves_cap, n_pick, max_leaves)) return rc;
    // the picks' counts, summed on the device before the cap rule cuts them, stay below 2^63
    const size_t eff_a = max_leaves_a < n_leaves_a ? max_leaves_a : n_leaves_a, eff_b = max_leaves_b < n_leaves_b ? max_leaves_b : n_leaves_b;
    if (n_trees_a > SIZE_MAX - n_trees_b || n_pick > (SIZE_MAX / 2) / (eff_a > eff_b ? eff_a : eff_b) || levels_cap > SIZE_MAX / 64)
        return refuse("size overflow");
    if (levels_cap < forest_levels_bound(arity, leaves_cap, n_pick, max_leaves))
        return refuse("levels_cap must be >= leaves_cap / (arity - 1) + n_pick * depth(max_leaves)");
    if (!d_leaves_a || !d_offsets_a || !d_roots_a || (max_leaves_a > 1 && !d_levels_a)) return refuse("NULL buffer of forest A");
    if (n_trees_b && (!d_leaves_b || !d_offsets_b || !d_roots_b || (max_leaves_b > 1 && !d_levels_b))) return refuse("NULL buffer of forest B");
    if (!d_pick) return refuse("NULL d_pick");
    if (!d_leaves_new || !d_offsets_new || !d_roots_new || (max_leaves > 1 && !d_levels_new)) return refuse("NULL output buffer");
    if (int rc = refuse.unless_aligned({d_leaves_a, d_levels_a, d_roots_a, d_leaves_b, d_levels_b, d_roots_b, d_leaves_new, d_levels_new, d_roots_new}))
        return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets_a), P252_NAMED(d_offsets_b), P252_NAMED(d_pick), P252_NAMED(d_offsets_new)}))
        return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    const size_t levels_a = forest_levels_bound(arity, n_leaves_a, n_trees_a, max_leaves_a);
    const size_t levels_b = forest_levels_bound(arity, n_leaves_b, n_trees_b, max_leaves_b);
    const ByteRange in[] = {{d_leaves_a, n_leaves_a * 32, "d_leaves_a"}, {d_offsets_a, (n_trees_a + 1) * 8, "d_offsets_a"},
                            {d_levels_a, levels_a * 32, "d_levels_a"},   {d_roots_a, n_trees_a * 32, "d_roots_a"},
                            {d_leaves_b, n_leaves_b * 32, "d_leaves_b"}, {d_offsets_b, n_trees_b ? (n_trees_b + 1) * 8 : 0, "d_offsets_b"},
                            {d_levels_b, levels_b * 32, "d_levels_b"},   {d_roots_b, n_trees_b * 32, "d_roots_b"},
                            {d_pick, n_pick * 8, "d_pick"}};
    const ByteRange out[] = {{d_leaves_new, leaves_cap * 32, "d_leaves_new"}, {d_offsets_new, (n_pick + 1) * 8, "d_offsets_new"},
                             {d_levels_new, levels_cap * 32, "d_levels_new"}, {d_roots_new, n_pick * 32, "d_roots_new"},
                             {d_n_bad, 4, "d_n_bad"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    ForestSelectSource A, B;
    A.leaves = d_leaves_a, A.offsets = d_offsets_a, A.levels = d_levels_a, A.roots = d_roots_a;
    A.n_leaves = n_leaves_a, A.n_trees = n_trees_a, A.max_leaves = max_leaves_a;
    B.leaves = d_leaves_b, B.offsets = d_offsets_b, B.levels = d_levels_b, B.roots = d_roots_b;
    B.n_leaves = n_leaves_b, B.n_trees = n_trees_b, B.max_leaves = max_leaves_b;
    const ForestSelectPlan plan = forest_select_plan(arity, n_trees_a, n_trees_b, max_leaves, n_pick, leaves_cap);
    return with_stream_scratch(ctx, refuse.who, st, plan.meta_bytes(), 0, [&](p252_ctx::LevelSet& set) {
        return launch_forest_select(plan, A, B, d_pick, d_leaves_new, d_offsets_new, d_levels_new, d_roots_new, d_n_bad, set.buf[0], st);
    });
}

P252_MERKLE_PAIR(int, forest_ragged_select_device_into,
                 (p252_ctx* ctx, const void* d_leaves_a, size_t n_leaves_a, const void* d_offsets_a, size_t n_trees_a, size_t max_leaves_a,
                  const void* d_levels_a, const void* d_roots_a, const void* d_leaves_b, size_t n_leaves_b, const void* d_offsets_b, size_t n_trees_b,
                  size_t max_leaves_b, const void* d_levels_b, const void* d_roots_b, const void* d_pick, size_t n_pick, void* d_leaves_new,
                  size_t leaves_cap, void* d_offsets_new, void* d_levels_new, size_t levels_cap, void* d_roots_new, void* d_n_bad, void* hip_stream),
                 forest_ragged_select_device_into(ctx, arity, d_leaves_a, n_leaves_a, d_offsets_a, n_trees_a, max_leaves_a, d_levels_a, d_roots_a,
                                                  d_leaves_b, n_leaves_b, d_offsets_b, n_trees_b, max_leaves_b, d_levels_b, d_roots_b, d_pick, n_pick,
                                                  d_leaves_new, leaves_cap, d_offsets_new, d_levels_new, levels_cap, d_roots_new, d_n_bad, hip_stream))

// ---- the shared proof of api.cpp's single tree across a forest of trees of DIFFERENT sizes (forest_multiproof.hip): k (tree id,
// leaf id) pairs behind one tree-major proof, every needed sibling stored once and every ancestor hashed once.  The scratch — the
// forest's index, the per-tree counters and the per-pair work lists in the first buffer; the verify's two lists of node values in
// the second — is the pair of the calling stream ----
P252_MERKLE_PAIR(size_t, forest_ragged_multiproof_bound, (size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k),
                 forest_multiproof_plan(arity, n_leaves, n_trees, max_leaves, k).bound)

static int forest_multiproof_shape_check(const Refusal& refuse, size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k) {
    if (k == 0 || n_trees == 0 || n_leaves == 0 || max_leaves == 0) return refuse("k, n_leaves, n_trees and max_leaves must be > 0");
    if (k > 0xffffffffu || max_leaves > 0xffffffffu) return refuse("k and max_leaves must be below 2^32 (a node index is a record word)");
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    return P252_OK;
}

static int forest_ragged_multiproof_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                           size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                           const void* d_leaf_ids, size_t k, void* d_leaves_out, void* d_proof, size_t proof_cap,
                                           void* d_proof_offsets, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_forest_ragged_multiproof" : "merkle2_forest_ragged_multiproof"};
    if (int rc = forest_multiproof_shape_check(refuse, n_leaves, n_trees, max_leaves, k)) return rc;
    const ForestMultiproofPlan plan = forest_multiproof_plan(arity, n_leaves, n_trees, max_leaves, k);
    if (!d_leaves || !d_offsets || !d_tree_ids || !d_leaf_ids || !d_leaves_out || !d_proof_offsets || (plan.depth && !d_levels) ||
        (proof_cap && !d_proof))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_proof})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_leaf_ids), P252_NAMED(d_proof_offsets)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_n_bad)})) return rc;
    if (proof_cap > SIZE_MAX / 32) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, plan.work_bytes(), 0, [&](p252_ctx::LevelSet& set) {
        return launch_forest_multiproof(plan, d_leaves, d_offsets, d_levels, d_tree_ids, d_leaf_ids, d_leaves_out, d_proof, proof_cap,
                                        d_proof_offsets, d_n_bad, set.buf[0], st);
    });
}

static int forest_ragged_multiproof_verify_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_offsets, size_t n_leaves,
                                                  size_t n_trees, size_t max_leaves, const void* d_tree_ids, const void* d_leaf_ids,
                                                  const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_len,
                                                  const void* d_proof_offsets, const void* d_roots, void* d_ok, void* d_roots_out,
                                                  void* d_n_hashed, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_forest_ragged_multiproof_verify" : "merkle2_forest_ragged_multiproof_verify"};
    if (int rc = forest_multiproof_shape_check(refuse, n_leaves, n_trees, max_leaves, k)) return rc;
    if (!tag || !d_offsets || !d_tree_ids || !d_leaf_ids || !d_leaves_in || !d_proof_offsets || !d_roots || !d_ok || (proof_len && !d_proof))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves_in, d_proof, d_roots, d_roots_out})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_leaf_ids), P252_NAMED(d_proof_offsets), P252_NAMED(d_n_hashed)}))
        return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_n_bad)})) return rc;
    if (proof_len > SIZE_MAX / 32) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestMultiproofPlan plan = forest_multiproof_plan(arity, n_leaves, n_trees, max_leaves, k);
    return with_stream_scratch(ctx, refuse.who, st, plan.work_bytes(), plan.values_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_forest_multiproof_verify(ctx->d_tab, tag_arg(tag), plan, d_offsets, d_tree_ids, d_leaf_ids, d_leaves_in, d_proof, proof_len,
                                               d_proof_offsets, d_roots, d_ok, d_roots_out, d_n_hashed, d_n_bad, set.buf[0], set.buf[1], st);
    });
}

P252_MERKLE_PAIR(int, forest_ragged_multiproof_device_into,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_leaves_out, void* d_proof, size_t proof_cap,
                  void* d_proof_offsets, void* d_n_bad, void* hip_stream),
                 forest_ragged_multiproof_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k,
                                                 d_leaves_out, d_proof, proof_cap, d_proof_offsets, d_n_bad, hip_stream))

P252_MERKLE_PAIR(int, forest_ragged_multiproof_verify_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_offsets, size_t n_leaves, size_t n_trees, size_t max_leaves,
                  const void* d_tree_ids, const void* d_leaf_ids, const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_len,
                  const void* d_proof_offsets, const void* d_roots, void* d_ok, void* d_roots_out, void* d_n_hashed, void* d_n_bad, void* hip_stream),
                 forest_ragged_multiproof_verify_device(ctx, arity, tag, d_offsets, n_leaves, n_trees, max_leaves, d_tree_ids, d_leaf_ids,
                                                        d_leaves_in, k, d_proof, proof_len, d_proof_offsets, d_roots, d_ok, d_roots_out, d_n_hashed,
                                                        d_n_bad, hip_stream))

// ---- a forest kept only as its frontiers (forest_frontier.hip): the append updates the caller's counts, rows and roots in place and
// hashes through the multiproof digest kernels; the extract takes that state out of a built forest.  The scratch — two words per tree,
// one scan row per level, the records and widths; the computed nodes of every level in the second buffer — is the pair of the calling
// stream ----
P252_MERKLE_PAIR(size_t, forest_frontier_bound, (size_t max_leaves), forest_frontier_stride(arity, max_leaves))

// the sizes of the state: n_trees x stride scalars inside size_t, the per-tree bookkeeping as in every forest call
static int forest_frontier_shape_check(const Refusal& refuse, unsigned arity, size_t n_trees, size_t max_leaves) {
    const size_t stride = forest_frontier_stride(arity, max_leaves);
    if (n_trees > SIZE_MAX / 8 / (FOREST_RAGGED_MAX_DEPTH + 2) || n_trees > SIZE_MAX / 64 / stride) return refuse("size overflow");
    return P252_OK;
}

// wit: the witnesses of p252_merkle{4,2}_forest_frontier_append_witness_device_into as the caller gave them (forest_witness.h).
// wit == nullptr or wit->k == 0: the plain append — the witness buffers are not looked at and nothing is launched for them
static int forest_frontier_append_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], void* d_counts, void* d_frontier, void* d_roots,
                                         size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add, const void* d_add_offsets,
                                         void* d_n_bad, void* d_n_hashed, const ForestWitnesses* wit, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const size_t k = wit ? wit->k : 0;
    if (n_trees == 0 && k == 0) return P252_OK;
    const Refusal refuse{ctx, k ? "merkle_forest_frontier_append_witness" : "merkle_forest_frontier_append"};
    if (max_leaves == 0) return refuse("max_leaves must be > 0");
    if (n_add > 0xffffffffull) return refuse("n_add must be below 2^32 (append in smaller chunks)");
    if (int rc = forest_frontier_shape_check(refuse, arity, n_trees, max_leaves)) return rc;
    if (n_trees > 0xffffffffull || (n_add && n_trees > (SIZE_MAX / 2) / n_add))  // (a record names its tree in 32 bits)
        return refuse("size overflow");
    // (a forest of no tree has no state to name: all of its witnesses are bad ones)
    if (!tag || (n_trees && (!d_counts || !d_frontier || !d_roots || !d_add_offsets)) || (n_add && !d_add)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_frontier, d_roots, d_add})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_counts), P252_NAMED(d_add_offsets), P252_NAMED(d_n_hashed)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    const size_t stride = forest_frontier_stride(arity, max_leaves);
    const ByteRange in[] = {{d_add, n_add * 32, "d_add"}, {d_add_offsets, n_trees ? (n_trees + 1) * 8 : 0, "d_add_offsets"}};
    const ByteRange out[] = {{d_counts, n_trees * 8, "d_counts"}, {d_frontier, n_trees * stride * 32, "d_frontier"},
                             {d_roots, n_trees * 32, "d_roots"},  {d_n_bad, 4, "d_n_bad"},
                             {d_n_hashed, 8, "d_n_hashed"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), false)) return rc;
    if (k) {
        const size_t depth = forest_ragged_depth(max_leaves, arity);
        if (!wit->tree_ids || !wit->leaf_ids || !wit->leaves || !wit->depths || (depth && (!wit->siblings || !wit->positions)))
            return refuse("NULL buffer");
        if (int rc = refuse.unless_aligned({wit->leaves, depth ? wit->siblings : nullptr})) return rc;
        if (int rc = refuse.unless_aligned(8, {{"d_wit_leaf_ids", wit->leaf_ids}})) return rc;
        if (int rc = refuse.unless_aligned(4, {{"d_wit_tree_ids", wit->tree_ids}, {"d_n_bad_witness", wit->n_bad}})) return rc;
        // k x D x (arity - 1) scalars inside size_t, and the blocks of the pass (floor(256 / D) witnesses each) inside a grid
        if (k > SIZE_MAX / 128 / (depth ? depth : 1) || forest_witness_blocks(k, (unsigned)depth) > 0x7fffffffull) return refuse("size overflow");
        // what the pass writes against everything the call reads or writes, and against each other
        const ByteRange mine[] = {{wit->leaves, k * 32, "d_wit_leaves"},
                                  {wit->siblings, k * depth * (arity - 1) * 32, "d_wit_siblings"},
                                  {wit->positions, k * depth, "d_wit_positions"},
                                  {wit->depths, k, "d_wit_depths"},
                                  {wit->n_bad, 4, "d_n_bad_witness"}};
        std::vector<ByteRange> others(out, out + std::size(out));
        others.insert(others.end(), in, in + std::size(in));
        others.push_back({wit->tree_ids, k * 4, "d_wit_tree_ids"});
        others.push_back({wit->leaf_ids, k * 8, "d_wit_leaf_ids"});
        if (int rc = refuse_overlaps(refuse, others.data(), others.size(), mine, std::size(mine), true)) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestFrontierPlan plan = forest_frontier_plan(arity, n_trees, max_leaves, n_add);
    if (n_trees == 0)  // (no scratch: one launch that marks every witness bad)
        return launched(ctx, refuse.who, launch_forest_frontier_append(ctx->d_tab, tag_arg(tag), plan, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                       nullptr, nullptr, nullptr, nullptr, wit, st));
    return with_stream_scratch(ctx, refuse.who, st, plan.work_bytes(), plan.value_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_forest_frontier_append(ctx->d_tab, tag_arg(tag), plan, d_counts, d_frontier, d_roots, d_add, d_add_offsets, d_n_bad,
                                             d_n_hashed, set.buf[0], set.buf[1], k ? wit : nullptr, st);
    });
}

P252_MERKLE_PAIR(int, forest_frontier_append_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier, void* d_roots, size_t n_trees, size_t max_leaves,
                  const void* d_add, size_t n_add, const void* d_add_offsets, void* d_n_bad, void* d_n_hashed, void* hip_stream),
                 forest_frontier_append_device(ctx, arity, tag, d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, n_add, d_add_offsets,
                                               d_n_bad, d_n_hashed, nullptr, hip_stream))

// the same append with the openings of k marked leaves kept current (forest_witness.hip): one launch more, inside the call
static int forest_frontier_append_witness_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], void* d_counts, void* d_frontier,
                                                            void* d_roots, size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add,
                                                            const void* d_add_offsets, const void* d_wit_tree_ids, const void* d_wit_leaf_ids,
                                                            size_t k, void* d_wit_leaves, void* d_wit_siblings, void* d_wit_positions,
                                                            void* d_wit_depths, void* d_n_bad, void* d_n_hashed, void* d_n_bad_witness,
                                                            void* hip_stream) {
    const ForestWitnesses wit = {static_cast<const uint32_t*>(d_wit_tree_ids), static_cast<const uint64_t*>(d_wit_leaf_ids), k, d_wit_leaves,
                                 d_wit_siblings, static_cast<uint8_t*>(d_wit_positions), static_cast<uint8_t*>(d_wit_depths),
                                 static_cast<unsigned*>(d_n_bad_witness)};
    return forest_frontier_append_device(ctx, arity, tag, d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, n_add, d_add_offsets, d_n_bad,
                                         d_n_hashed, &wit, hip_stream);
}

P252_MERKLE_PAIR(int, forest_frontier_append_witness_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier, void* d_roots, size_t n_trees, size_t max_leaves,
                  const void* d_add, size_t n_add, const void* d_add_offsets, const void* d_wit_tree_ids, const void* d_wit_leaf_ids, size_t k,
                  void* d_wit_leaves, void* d_wit_siblings, void* d_wit_positions, void* d_wit_depths, void* d_n_bad, void* d_n_hashed,
                  void* d_n_bad_witness, void* hip_stream),
                 forest_frontier_append_witness_device(ctx, arity, tag, d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, n_add,
                                                       d_add_offsets, d_wit_tree_ids, d_wit_leaf_ids, k, d_wit_leaves, d_wit_siblings,
                                                       d_wit_positions, d_wit_depths, d_n_bad, d_n_hashed, d_n_bad_witness, hip_stream))

static int forest_frontier_extract_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                          size_t n_trees, size_t max_leaves_forest, const void* d_levels, const void* d_roots_forest,
                                          size_t max_leaves, void* d_counts, void* d_frontier, void* d_roots, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (n_trees == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_frontier_extract"};
    if (max_leaves_forest == 0 || max_leaves < max_leaves_forest) return refuse("max_leaves_forest must be > 0 and max_leaves >= max_leaves_forest");
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves_forest)) return rc;
    if (int rc = forest_frontier_shape_check(refuse, arity, n_trees, max_leaves)) return rc;
    if (!d_leaves || !d_offsets || !d_roots_forest || !d_counts || !d_frontier || !d_roots || (max_leaves_forest > 1 && !d_levels))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_roots_forest, d_frontier, d_roots})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_counts)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    const size_t stride = forest_frontier_stride(arity, max_leaves);
    const size_t levels_forest = forest_levels_bound(arity, n_leaves, n_trees, max_leaves_forest);
    const ByteRange in[] = {{d_leaves, n_leaves * 32, "d_leaves"},
                            {d_offsets, (n_trees + 1) * 8, "d_offsets"},
                            {d_levels, levels_forest * 32, "d_levels"},
                            {d_roots_forest, n_trees * 32, "d_roots_forest"}};
    const ByteRange out[] = {{d_counts, n_trees * 8, "d_counts"}, {d_frontier, n_trees * stride * 32, "d_frontier"},
                             {d_roots, n_trees * 32, "d_roots"},  {d_n_bad, 4, "d_n_bad"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), false)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, forest_ragged_index_bytes(n_trees), 0, [&](p252_ctx::LevelSet& set) {
        return launch_forest_frontier_extract(arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots_forest,
                                              max_leaves, d_counts, d_frontier, d_roots, d_n_bad, set.buf[0], st);
    });
}

P252_MERKLE_PAIR(int, forest_frontier_extract_device_into,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves_forest,
                  const void* d_levels, const void* d_roots_forest, size_t max_leaves, void* d_counts, void* d_frontier, void* d_roots, void* d_n_bad,
                  void* hip_stream),
                 forest_frontier_extract_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots_forest,
                                                max_leaves, d_counts, d_frontier, d_roots, d_n_bad, hip_stream))

// ---- consistency proofs of a ragged forest (forest_consistency.hip): that a tree of m leaves is the tree it was at n <= m leaves with
// leaves appended.  The extraction takes the forest's index and the proof records in the scratch pair of the calling stream, as the
// openings call does; the verification the old chain's openings, both recomputed roots, the sort's order and counters ----
static int forest_ragged_consistency_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                            size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                            const void* d_old_counts, size_t k, void* d_new_counts_out, void* d_leaves_out, void* d_siblings,
                                            void* d_positions, void* d_depths, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_ragged_consistency"};
    if (int rc = refuse.unless_built_forest(n_leaves, n_trees, max_leaves)) return rc;
    const size_t depth = forest_ragged_depth(max_leaves, arity);
    if (!d_leaves || !d_offsets || !d_tree_ids || !d_old_counts || !d_new_counts_out || !d_leaves_out || !d_depths ||
        (depth && (!d_levels || !d_siblings || !d_positions)))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_siblings})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_old_counts), P252_NAMED(d_new_counts_out)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    if (k > SIZE_MAX / 128 / (depth ? depth : 1)) return refuse("size overflow");
    const size_t levels_forest = forest_levels_bound(arity, n_leaves, n_trees, max_leaves);
    const ByteRange in[] = {{d_leaves, n_leaves * 32, "d_leaves"},
                            {d_offsets, (n_trees + 1) * 8, "d_offsets"},
                            {d_levels, levels_forest * 32, "d_levels"},
                            {d_tree_ids, k * 4, "d_tree_ids"},
                            {d_old_counts, k * 8, "d_old_counts"}};
    const ByteRange out[] = {{d_new_counts_out, k * 8, "d_new_counts_out"},
                             {d_leaves_out, k * 32, "d_leaves_out"},
                             {d_siblings, k * depth * (arity - 1) * 32, "d_siblings"},
                             {d_positions, k * depth, "d_positions"},
                             {d_depths, k, "d_depths"},
                             {d_n_bad, 4, "d_n_bad"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, forest_openings_record_bytes(k), 0,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* records, void*) {
                                 return launch_forest_consistency_extract(arity, d_leaves, d_levels, d_offsets, ntree, lo, n_trees, d_tree_ids,
                                                                          d_old_counts, k, (unsigned)depth, records, d_new_counts_out, d_leaves_out,
                                                                          d_siblings, d_positions, d_depths, d_n_bad, st);
                             });
}

static int forest_consistency_verify_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_old_counts,
                                            const void* d_old_roots, const void* d_new_counts, const void* d_new_roots, const void* d_leaves_in,
                                            const void* d_siblings, const void* d_positions, const void* d_depths, size_t stride_depth, size_t k,
                                            const void* d_tree_ids, size_t n_trees, void* d_ok, void* d_old_roots_out, void* d_new_roots_out,
                                            void* d_n_hashed, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_consistency_verify"};
    if (int rc = path_ragged_check(refuse, tag, d_leaves_in, d_siblings, d_positions, d_depths, stride_depth, k)) return rc;
    const size_t n_claims = d_tree_ids ? n_trees : k;  // (a forest of no tree has no claim to name: all of its proofs are refused)
    if (!d_ok || (n_claims && (!d_old_counts || !d_old_roots || !d_new_counts || !d_new_roots))) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_old_roots, d_new_roots, d_old_roots_out, d_new_roots_out})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_old_counts), P252_NAMED(d_new_counts), P252_NAMED(d_n_hashed)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids)})) return rc;
    // the claims, and the work area (two openings, two roots and the order per proof), inside size_t
    if (n_claims > SIZE_MAX / 64 || k > SIZE_MAX / 512 / (stride_depth ? stride_depth : 1)) return refuse("size overflow");
    const ByteRange in[] = {{d_old_counts, n_claims * 8, "d_old_counts"},
                            {d_old_roots, n_claims * 32, "d_old_roots"},
                            {d_new_counts, n_claims * 8, "d_new_counts"},
                            {d_new_roots, n_claims * 32, "d_new_roots"},
                            {d_leaves_in, k * 32, "d_leaves_in"},
                            {d_siblings, k * stride_depth * (arity - 1) * 32, "d_siblings"},
                            {d_positions, k * stride_depth, "d_positions"},
                            {d_depths, k, "d_depths"},
                            {d_tree_ids, k * 4, "d_tree_ids"}};
    const ByteRange out[] = {{d_ok, k, "d_ok"},
                             {d_old_roots_out, k * 32, "d_old_roots_out"},
                             {d_new_roots_out, k * 32, "d_new_roots_out"},
                             {d_n_hashed, 8, "d_n_hashed"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const bool sort = ragged_sort_enabled();  // P252_RAGGED_SORT=0: identity order
    return with_stream_scratch(ctx, refuse.who, st, forest_consistency_work(arity, k, (unsigned)stride_depth).bytes, forest_openings_hist_bytes(),
                               [&](p252_ctx::LevelSet& set) {
                                   return launch_forest_consistency_verify(arity, ctx->d_tab, tag_arg(tag), d_old_counts, d_old_roots, d_new_counts,
                                                                           d_new_roots, d_leaves_in, d_siblings, d_positions, d_depths,
                                                                           (unsigned)stride_depth, k, d_tree_ids, n_trees, d_ok, d_old_roots_out,
                                                                           d_new_roots_out, d_n_hashed, set.buf[0], set.buf[1], sort, st);
                               });
}

P252_MERKLE_PAIR(int, forest_ragged_consistency_device_into,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  const void* d_levels, const void* d_tree_ids, const void* d_old_counts, size_t k, void* d_new_counts_out, void* d_leaves_out,
                  void* d_siblings, void* d_positions, void* d_depths, void* d_n_bad, void* hip_stream),
                 forest_ragged_consistency_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_old_counts,
                                                  k, d_new_counts_out, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad, hip_stream))

P252_MERKLE_PAIR(int, forest_consistency_verify_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_old_counts, const void* d_old_roots, const void* d_new_counts,
                  const void* d_new_roots, const void* d_leaves_in, const void* d_siblings, const void* d_positions, const void* d_depths,
                  size_t stride_depth, size_t k, const void* d_tree_ids, size_t n_trees, void* d_ok, void* d_old_roots_out, void* d_new_roots_out,
                  void* d_n_hashed, void* hip_stream),
                 forest_consistency_verify_device(ctx, arity, tag, d_old_counts, d_old_roots, d_new_counts, d_new_roots, d_leaves_in, d_siblings,
                                                  d_positions, d_depths, stride_depth, k, d_tree_ids, n_trees, d_ok, d_old_roots_out, d_new_roots_out,
                                                  d_n_hashed, hip_stream))

// ---- roots and openings of such a forest's trees as they were at earlier leaf counts (forest_anchor.hip): m anchors (tree, count), k
// openings (anchor, leaf).  The scratch — the forest's index, a record per anchor, the partial nodes of every anchor and level, a record
// per opening; one level's gathered children in the second buffer — is the pair of the calling stream ----
static int forest_ragged_anchor_openings_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                const void* d_anchor_tree_ids, const void* d_anchor_counts, size_t m, const void* d_anchor_ids,
                                                const void* d_leaf_ids, size_t k, void* d_anchor_roots, void* d_anchor_depths,
                                                void* d_leaves_out, void* d_siblings, void* d_positions, void* d_depths, void* d_n_bad_anchors,
                                                void* d_n_bad, void* d_n_hashed, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (m == 0 && k == 0) return P252_OK;
    const Refusal refuse{ctx, "merkle_forest_ragged_anchor_openings"};
    if (int rc = refuse.unless_built_forest(n_leaves, n_trees, max_leaves)) return rc;
    const size_t depth = forest_ragged_depth(max_leaves, arity);
    if (!tag || !d_leaves || !d_offsets || (depth && !d_levels) ||
        (m && (!d_anchor_tree_ids || !d_anchor_counts || !d_anchor_roots || !d_anchor_depths)) ||
        (k && (!d_anchor_ids || !d_leaf_ids || !d_leaves_out || !d_depths || (depth && (!d_siblings || !d_positions)))))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_anchor_roots, d_leaves_out, d_siblings})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_anchor_counts), P252_NAMED(d_leaf_ids), P252_NAMED(d_n_hashed)}))
        return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_anchor_tree_ids), P252_NAMED(d_anchor_ids), P252_NAMED(d_n_bad_anchors), P252_NAMED(d_n_bad)}))
        return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    // an anchor id is 32 bits; the partial nodes (m x D scalars) and the openings (k x D x (arity - 1) scalars) inside size_t
    if (m > 0xffffffffull || m > SIZE_MAX / 256 / (depth ? depth : 1) || k > SIZE_MAX / 128 / (depth ? depth : 1)) return refuse("size overflow");
    const size_t levels_forest = forest_levels_bound(arity, n_leaves, n_trees, max_leaves);
    const ByteRange in[] = {{d_leaves, n_leaves * 32, "d_leaves"},
                            {d_offsets, (n_trees + 1) * 8, "d_offsets"},
                            {d_levels, levels_forest * 32, "d_levels"},
                            {d_anchor_tree_ids, m * 4, "d_anchor_tree_ids"},
                            {d_anchor_counts, m * 8, "d_anchor_counts"},
                            {d_anchor_ids, k * 4, "d_anchor_ids"},
                            {d_leaf_ids, k * 8, "d_leaf_ids"}};
    const ByteRange out[] = {{d_anchor_roots, m * 32, "d_anchor_roots"},
                             {d_anchor_depths, m, "d_anchor_depths"},
                             {d_leaves_out, k * 32, "d_leaves_out"},
                             {d_siblings, k * depth * (arity - 1) * 32, "d_siblings"},
                             {d_positions, k * depth, "d_positions"},
                             {d_depths, k, "d_depths"},
                             {d_n_bad_anchors, 4, "d_n_bad_anchors"},
                             {d_n_bad, 4, "d_n_bad"},
                             {d_n_hashed, 8, "d_n_hashed"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestAnchorWork w = forest_anchor_work(arity, m, k, (unsigned)depth);
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, w.bytes, w.children_bytes,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* work, void* children) {
                                 return launch_forest_anchor_openings(arity, ctx->d_tab, tag_arg(tag), d_leaves, d_levels, d_offsets, ntree, lo,
                                                                      n_trees, d_anchor_tree_ids, d_anchor_counts, m, d_anchor_ids, d_leaf_ids, k,
                                                                      (unsigned)depth, d_anchor_roots, d_anchor_depths, d_leaves_out, d_siblings,
                                                                      d_positions, d_depths, d_n_bad_anchors, d_n_bad, d_n_hashed, work, children,
                                                                      st);
                             });
}

P252_MERKLE_PAIR(int, forest_ragged_anchor_openings_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                  size_t max_leaves, const void* d_levels, const void* d_anchor_tree_ids, const void* d_anchor_counts, size_t m,
                  const void* d_anchor_ids, const void* d_leaf_ids, size_t k, void* d_anchor_roots, void* d_anchor_depths, void* d_leaves_out,
                  void* d_siblings, void* d_positions, void* d_depths, void* d_n_bad_anchors, void* d_n_bad, void* d_n_hashed, void* hip_stream),
                 forest_ragged_anchor_openings_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels,
                                                      d_anchor_tree_ids, d_anchor_counts, m, d_anchor_ids, d_leaf_ids, k, d_anchor_roots,
                                                      d_anchor_depths, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad_anchors, d_n_bad,
                                                      d_n_hashed, hip_stream))

// ---- whole runs of leaves of such a forest's trees proved and checked in one call (forest_range.hip): m runs [first, first + len) with
// their k leaves flat behind d_leaf_offsets.  The proofs are closed forms, so the extraction is the forest's index, the runs' index
// and a gather; the verification needs no forest: the runs' index, one count and one scan row per level, the records and widths of
// one level in the first buffer, two lists of node values in the second — the pair of the calling stream ----
P252_MERKLE_PAIR(size_t, forest_range_stride, (size_t max_leaves), forest_range_stride(arity, max_leaves))

// what both calls ask of (m, k, max_leaves): a run start in a value list and a node index are 32-bit record words
static int forest_range_shape_check(const Refusal& refuse, size_t m, size_t k, size_t max_leaves, size_t n_trees) {
    if (m == 0 || k == 0 || max_leaves == 0 || n_trees == 0) return refuse("m, k, n_trees and max_leaves must be > 0");
    if (k > 0xffffffffu || m > 0xffffffffu || max_leaves > 0xffffffffu || (uint64_t)k + 2 * (uint64_t)m > 0xffffffffu)
        return refuse("k, m, k + 2 m and max_leaves must be below 2^32 (record words are 32-bit)");
    return P252_OK;
}

static int forest_ragged_range_proofs_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                             size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                             const void* d_first, const void* d_leaf_offsets, size_t m, size_t k, void* d_leaves_out,
                                             void* d_proof, void* d_proof_lens, void* d_counts_out, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_forest_ragged_range_proofs" : "merkle2_forest_ragged_range_proofs"};
    if (n_leaves == 0) return refuse("n_leaves must be > 0");
    if (int rc = forest_range_shape_check(refuse, m, k, max_leaves, n_trees)) return rc;
    const size_t stride = forest_range_stride(arity, max_leaves);
    if (!d_leaves || !d_offsets || !d_tree_ids || !d_first || !d_leaf_offsets || !d_proof_lens || !d_counts_out ||
        (stride && (!d_levels || !d_proof)))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_proof})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_first), P252_NAMED(d_leaf_offsets), P252_NAMED(d_counts_out)}))
        return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_proof_lens), P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestRangePlan plan = forest_range_plan(arity, max_leaves, m, k);
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, plan.extract_bytes, 0,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* work, void*) {
                                 return launch_forest_range_proofs(plan, d_leaves, d_offsets, d_levels, ntree, lo, n_trees, d_tree_ids, d_first,
                                                                   d_leaf_offsets, d_leaves_out, d_proof, d_proof_lens, d_counts_out, d_n_bad,
                                                                   work, st);
                             });
}

static int forest_range_verify_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_tree_ids, const void* d_counts,
                                      const void* d_first, const void* d_leaf_offsets, size_t m, size_t max_leaves, const void* d_leaves_in,
                                      size_t k, const void* d_proof, size_t proof_stride, const void* d_proof_lens, const void* d_roots,
                                      size_t n_trees, void* d_ok, void* d_roots_out, void* d_n_hashed, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_forest_range_verify" : "merkle2_forest_range_verify"};
    if (int rc = forest_range_shape_check(refuse, m, k, max_leaves, n_trees)) return rc;
    if (!tag || !d_tree_ids || !d_counts || !d_first || !d_leaf_offsets || !d_leaves_in || !d_proof_lens || !d_roots || !d_ok ||
        (proof_stride && !d_proof))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves_in, d_proof, d_roots, d_roots_out})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_counts), P252_NAMED(d_first), P252_NAMED(d_leaf_offsets), P252_NAMED(d_n_hashed)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_proof_lens), P252_NAMED(d_n_bad)})) return rc;
    // a proof offset (row times stride, plus a place in the row) is 60 bits of a record; the rows' bytes inside size_t
    if (n_trees > SIZE_MAX / 32 || (proof_stride && m > (SIZE_MAX >> 8) / proof_stride)) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestRangePlan plan = forest_range_plan(arity, max_leaves, m, k);
    return with_stream_scratch(ctx, refuse.who, st, plan.verify_bytes, plan.values_bytes, [&](p252_ctx::LevelSet& set) {
        return launch_forest_range_verify(ctx->d_tab, tag_arg(tag), plan, d_tree_ids, d_counts, d_first, d_leaf_offsets, d_leaves_in, d_proof,
                                          proof_stride, d_proof_lens, d_roots, n_trees, d_ok, d_roots_out, d_n_hashed, d_n_bad, set.buf[0],
                                          set.buf[1], st);
    });
}

P252_MERKLE_PAIR(int, forest_ragged_range_proofs_device_into,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  const void* d_levels, const void* d_tree_ids, const void* d_first, const void* d_leaf_offsets, size_t m, size_t k,
                  void* d_leaves_out, void* d_proof, void* d_proof_lens, void* d_counts_out, void* d_n_bad, void* hip_stream),
                 forest_ragged_range_proofs_device(ctx, arity, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_first,
                                                   d_leaf_offsets, m, k, d_leaves_out, d_proof, d_proof_lens, d_counts_out, d_n_bad, hip_stream))

P252_MERKLE_PAIR(int, forest_range_verify_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_tree_ids, const void* d_counts, const void* d_first, const void* d_leaf_offsets,
                  size_t m, size_t max_leaves, const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_stride, const void* d_proof_lens,
                  const void* d_roots, size_t n_trees, void* d_ok, void* d_roots_out, void* d_n_hashed, void* d_n_bad, void* hip_stream),
                 forest_range_verify_device(ctx, arity, tag, d_tree_ids, d_counts, d_first, d_leaf_offsets, m, max_leaves, d_leaves_in, k, d_proof,
                                            proof_stride, d_proof_lens, d_roots, n_trees, d_ok, d_roots_out, d_n_hashed, d_n_bad, hip_stream))

// ---- leaf updates of such a forest applied in order, each with its witness (forest_sequential.hip).  The scratch — the forest's
// index, two sorted lists of keys and values, the parents' values and the rank words; one level's gathered children in the second
// buffer — is the pair of the calling stream ----
static int forest_ragged_update_sequential_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                  const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                  const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, const void* d_order,
                                                  size_t k, void* d_old_leaves, void* d_siblings, void* d_positions, void* d_depths,
                                                  void* d_roots_before, void* d_roots_after, void* d_roots, void* d_n_bad, void* d_n_hashed,
                                                  void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_forest_ragged_update_sequential" : "merkle2_forest_ragged_update_sequential"};
    if (k == 0 || max_leaves == 0 || n_trees == 0 || n_leaves == 0) return refuse("k, n_leaves, n_trees and max_leaves must be > 0");
    if (k > 0xffffffffu || max_leaves > 0xffffffffu) return refuse("k and max_leaves must be below 2^32 (an index and a node are 32-bit words)");
    const size_t depth = forest_ragged_depth(max_leaves, arity);
    if (!tag || !d_leaves || !d_offsets || !d_tree_ids || !d_leaf_ids || !d_new_leaves || !d_order || !d_depths || !d_roots_after ||
        (depth && (!d_levels || !d_siblings || !d_positions)))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_new_leaves, d_old_leaves, d_siblings, d_roots_before, d_roots_after, d_roots}))
        return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets), P252_NAMED(d_leaf_ids), P252_NAMED(d_n_hashed)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids), P252_NAMED(d_order), P252_NAMED(d_n_bad)})) return rc;
    if (int rc = forest_shape_check(refuse, n_leaves, n_trees, max_leaves)) return rc;  // (the build's own limits)
    const size_t levels_forest = forest_levels_bound(arity, n_leaves, n_trees, max_leaves);
    const ByteRange in[] = {{d_leaves, n_leaves * 32, "d_leaves"},
                            {d_offsets, (n_trees + 1) * 8, "d_offsets"},
                            {d_levels, levels_forest * 32, "d_levels"},
                            {d_roots, n_trees * 32, "d_roots"},
                            {d_tree_ids, k * 4, "d_tree_ids"},
                            {d_leaf_ids, k * 8, "d_leaf_ids"},
                            {d_new_leaves, k * 32, "d_new_leaves"},
                            {d_order, k * 4, "d_order"}};
    const ByteRange out[] = {{d_old_leaves, k * 32, "d_old_leaves"},
                             {d_siblings, k * depth * (arity - 1) * 32, "d_siblings"},
                             {d_positions, k * depth, "d_positions"},
                             {d_depths, k, "d_depths"},
                             {d_roots_before, k * 32, "d_roots_before"},
                             {d_roots_after, k * 32, "d_roots_after"},
                             {d_n_bad, 4, "d_n_bad"},
                             {d_n_hashed, 8, "d_n_hashed"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const ForestSequentialWork w = forest_sequential_work(arity, k);
    return with_forest_index(ctx, refuse.who, st, arity, d_offsets, n_trees, n_leaves, max_leaves, w.bytes, depth ? w.children_bytes : 0,
                             [&](const uint64_t* ntree, const uint64_t* lo, char* work, void* children) {
                                 return launch_forest_update_sequential(arity, ctx->d_tab, tag_arg(tag), d_leaves, d_offsets, ntree, lo, n_trees,
                                                                        d_levels, d_tree_ids, d_leaf_ids, d_new_leaves, d_order, k,
                                                                        (unsigned)depth, d_old_leaves, d_siblings, d_positions, d_depths,
                                                                        d_roots_before, d_roots_after, d_roots, d_n_bad, d_n_hashed, work,
                                                                        children, st);
                             });
}

P252_MERKLE_PAIR(int, forest_ragged_update_sequential_device_into,
                 (p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees, size_t max_leaves,
                  void* d_levels, const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, const void* d_order, size_t k,
                  void* d_old_leaves, void* d_siblings, void* d_positions, void* d_depths, void* d_roots_before, void* d_roots_after, void* d_roots,
                  void* d_n_bad, void* d_n_hashed, void* hip_stream),
                 forest_ragged_update_sequential_device(ctx, arity, tag, d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids,
                                                        d_leaf_ids, d_new_leaves, d_order, k, d_old_leaves, d_siblings, d_positions, d_depths,
                                                        d_roots_before, d_roots_after, d_roots, d_n_bad, d_n_hashed, hip_stream))

// ---- the order and the distinct pairs the calls above take, made on the device (pairs.hip): neither depends on an arity.  The
// scratch — the plan, two arrays of records and the per-tile digit counts — is the first buffer of the calling stream's pair ----
static int pairs_common_check(const Refusal& refuse, const void* d_tree_ids, const void* d_leaf_ids, size_t k) {
    if (k == 0) return refuse("k must be > 0");
    if (k > 0xffffffffu) return refuse("k must be below 2^32 (an index is a 32-bit word)");
    if (!d_leaf_ids) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_leaf_ids)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids)})) return rc;
    if (pairs_work(k).bytes > SIZE_MAX / 2) return refuse("size overflow");  // (never, below 2^32)
    return P252_OK;
}

int p252_pairs_order_device_into(p252_ctx* ctx, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_order, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "pairs_order"};
    if (int rc = pairs_common_check(refuse, d_tree_ids, d_leaf_ids, k)) return rc;
    if (!d_order) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_order)})) return rc;
    const ByteRange in[] = {{d_tree_ids, k * 4, "d_tree_ids"}, {d_leaf_ids, k * 8, "d_leaf_ids"}};
    const ByteRange out[] = {{d_order, k * 4, "d_order"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, pairs_work(k).bytes, 0, [&](p252_ctx::LevelSet& set) {
        return launch_pairs_order(d_tree_ids, d_leaf_ids, k, d_order, set.buf[0], st);
    });
}

int p252_pairs_unique_device_into(p252_ctx* ctx, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_tree_ids_out,
                                  void* d_leaf_ids_out, void* d_indices_out, void* d_first, void* d_n_unique, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "pairs_unique"};
    if (int rc = pairs_common_check(refuse, d_tree_ids, d_leaf_ids, k)) return rc;
    if (!d_n_unique) return refuse("NULL buffer");
    if (!d_tree_ids_out && !d_leaf_ids_out && !d_indices_out && !d_first)
        return refuse("at least one of d_tree_ids_out, d_leaf_ids_out, d_indices_out and d_first must be given");
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_leaf_ids_out), P252_NAMED(d_n_unique)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_tree_ids_out), P252_NAMED(d_indices_out), P252_NAMED(d_first)})) return rc;
    const ByteRange in[] = {{d_tree_ids, k * 4, "d_tree_ids"}, {d_leaf_ids, k * 8, "d_leaf_ids"}};
    const ByteRange out[] = {{d_tree_ids_out, k * 4, "d_tree_ids_out"},
                             {d_leaf_ids_out, k * 8, "d_leaf_ids_out"},
                             {d_indices_out, k * 4, "d_indices_out"},
                             {d_first, k * 4, "d_first"},
                             {d_n_unique, 8, "d_n_unique"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, pairs_work(k).bytes, 0, [&](p252_ctx::LevelSet& set) {
        return launch_pairs_unique(d_tree_ids, d_leaf_ids, k, d_tree_ids_out, d_leaf_ids_out, d_indices_out, d_first, d_n_unique, set.buf[0], st);
    });
}

}  // (the C ABI)
