// forest_consistency.h — launch interface between api_forest.cpp and forest_consistency.hip: the proof that a tree of a ragged forest, now
// of m leaves, is the tree it was at n <= m leaves with leaves appended and nothing before them changed
// (p252_merkle{4,2}_forest_ragged_consistency_device_into), and its check against the two roots
// (p252_merkle{4,2}_forest_consistency_verify_device_into).  The proof of (tree t, old count n) is the opening of leaf index n of the
// tree as it is now, in the layout of forest_openings.h: with A = arity, f_l(n) = n / A^l and d_l(n) = f_l(n) % A its slot on row l
// is d_l(n), and its siblings left of that slot are the nodes [A f_{l+1}(n), f_l(n)) of level l — row l of the frontier of the tree
// at n leaves.  The whole opening re-hashes to the new root; its left siblings alone re-hash to the old one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

// extraction, no hashing: ntree / lo = the forest's index (launch_forest_ragged_index), records = forest_openings_record_bytes(k) of
// scratch.  With n_t the leaves of tree tree_ids[i] and n = old_counts[i]: 1 <= n < n_t — the opening of (t, leaf n) as
// launch_forest_openings writes it, new_counts_out[i] = n_t; n == n_t — zeros, depths[i] = depth(n_t), new_counts_out[i] = n_t; a
// bad proof (tree id >= n_trees, a bad tree, n == 0, n > n_t) — zeros, depth 0xFF, new count 0, counted once in *n_bad (device
// uint32, may be null).  leaves must hold at least one scalar.
hipError_t launch_forest_consistency_extract(unsigned arity, const void* leaves, const void* levels, const void* offsets,
                                             const uint64_t* ntree, const uint64_t* lo, size_t n_trees, const void* tree_ids,
                                             const void* old_counts, size_t k, unsigned stride_depth, void* records, void* new_counts_out,
                                             void* leaves_out, void* siblings, void* positions, void* depths, void* n_bad, hipStream_t st);

// the work area of the verification: the old chain's opening (leaf, rows, slots, depth), the new chain's slots and depth, a status
// byte, both recomputed roots and the sort's order — offsets into one buffer of `bytes` bytes, the 16-byte parts first
struct ForestConsistencyWork {
    size_t o_leaves, o_sib, got_old, got_new, order, o_pos, n_pos, o_dep, n_dep, status, bytes;
};
inline ForestConsistencyWork forest_consistency_work(unsigned arity, size_t k, unsigned stride_depth) {
    ForestConsistencyWork w{};
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    };
    w.o_leaves = take(k * 32);
    w.o_sib = take(k * stride_depth * (arity - 1) * 32);
    w.got_old = take(k * 32);
    w.got_new = take(k * 32);
    w.order = take(k * sizeof(uint64_t));
    w.o_pos = take(k * stride_depth);
    w.n_pos = take(k * stride_depth);
    w.o_dep = take(k);
    w.n_dep = take(k);
    w.status = take(k);
    w.bytes = at;
    return w;
}

// verification.  Claim c of proof i: c = i (tree_ids == null, the claim arrays hold k entries) or c = tree_ids[i] (they hold
// n_claims; c >= n_claims is refused).  ok[i] = 1 iff 1 <= n <= m, depths[i] == depth(m) <= stride_depth and — n == m — the two
// claimed roots are the same bytes (nothing hashed, the opening not read; the roots out are the claimed ones) or — n < m —
// positions[i][l] == d_l(n) for l < depth(m), the whole opening re-hashes to new_roots[c] and its left siblings to old_roots[c].
// old_roots_out / new_roots_out (may be null): the recomputed roots, zero for a refused proof.  *n_hashed (device uint64, may be
// null) gains the digests computed.  work = forest_consistency_work(..).bytes of scratch, hist = forest_openings_hist_bytes();
// sort == false: the identity order.
hipError_t launch_forest_consistency_verify(unsigned arity, const int32_t* tab, const TagArg& tag, const void* old_counts,
                                            const void* old_roots, const void* new_counts, const void* new_roots, const void* leaves,
                                            const void* siblings, const void* positions, const void* depths, unsigned stride_depth, size_t k,
                                            const void* tree_ids, size_t n_claims, void* ok, void* old_roots_out, void* new_roots_out,
                                            void* n_hashed, void* work, void* hist, bool sort, hipStream_t st);

}  // namespace p252
