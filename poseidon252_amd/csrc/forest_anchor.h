// forest_anchor.h — launch interface between api_forest.cpp and forest_anchor.hip: roots and openings of the trees of a built ragged
// forest AS THEY WERE at earlier leaf counts (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into).  An anchor is (tree t, count
// c <= n_t); with A = arity and f_l(c) = c / A^l, node j of level l of the tree at c leaves is the stored node while j < f_l(c), the
// PARTIAL node P_l(c) at j == f_l(c) when c % A^l != 0, and nothing right of that.  P_l(c) = H(the stored nodes [A f_l(c), f_{l-1}(c))
// of level l - 1, then P_{l-1}(c) if it exists, then zeros); the root at c is P_depth(c)(c), or the stored node when c == A^depth(c).
// The openings are in the layout of forest_openings.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace p252 {

// the work area of a call with m anchors and k openings at stride D: one 32-byte record per anchor, the partial nodes P[l - 1][a]
// (level-major, so that a level's digests are one contiguous output), one 48-byte record per opening — offsets into the first scratch
// buffer behind the forest's index; the second buffer holds one level's gathered children, m x arity scalars
struct ForestAnchorWork {
    size_t anchors, partial, records, bytes, children_bytes;
};
inline ForestAnchorWork forest_anchor_work(unsigned arity, size_t m, size_t k, unsigned stride_depth) {
    ForestAnchorWork w{};
    w.anchors = 0;
    w.partial = w.anchors + m * 32;
    w.records = w.partial + m * stride_depth * 32;
    w.bytes = w.records + k * 48;
    w.children_bytes = stride_depth ? m * arity * 32 : 0;
    return w;
}

// ntree / lo = the forest's index (launch_forest_ragged_index); work / children = the two areas above.  Anchor a = (anchor_tree_ids[a],
// anchor_counts[a]) is valid iff the tree is known and good and 1 <= c <= n_t: anchor_roots[a] = the root of the tree's first c leaves,
// anchor_depths[a] = depth(c), *n_hashed (device uint64, may be null) gains depth(c) - (the lowest level whose digit of c is not zero).
// A bad anchor: a zero root, depth 0xFF, one count in *n_bad_anchors (device uint32, may be null).  Opening i = leaf leaf_ids[i] under
// anchor anchor_ids[i], valid iff the id is < m, the anchor valid and the leaf id < c: what launch_forest_openings writes for that leaf on
// a forest built from the tree's first c leaves; a bad one is zeros with depth 0xFF, counted once in *n_bad.  k == 0: the anchors alone.
// The digests are launch_merkle4's, one launch of m nodes per level over children gathered by k_fa_children.
hipError_t launch_forest_anchor_openings(unsigned arity, const int32_t* tab, const TagArg& tag, const void* leaves, const void* levels,
                                         const void* offsets, const uint64_t* ntree, const uint64_t* lo, size_t n_trees,
                                         const void* anchor_tree_ids, const void* anchor_counts, size_t m, const void* anchor_ids,
                                         const void* leaf_ids, size_t k, unsigned stride_depth, void* anchor_roots, void* anchor_depths,
                                         void* leaves_out, void* siblings, void* positions, void* depths, void* n_bad_anchors, void* n_bad,
                                         void* n_hashed, void* work, void* children, hipStream_t st);

}  // namespace p252
