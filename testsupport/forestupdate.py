"""The numpy model of what one leaf update of a ragged forest (p252_merkle{4,2}_forest_ragged_update_device) may hash;
tests/test_forest_update_cpu.py checks it.  No torch here: the CPU tests import it too."""
import numpy as np

from .treeshape import depth


def dirty_nodes(sizes, tree_ids, leaf_ids, arity):
    """the number of DISTINCT nodes above the leaves (tree_ids[i], leaf_ids[i]) of a forest of trees of `sizes` leaves: what one call
    may hash.  Bad updates (tree id outside the forest, an empty tree, leaf id outside the tree) dirty nothing."""
    sizes = np.asarray(sizes, dtype=np.int64)
    tid, lid = np.asarray(tree_ids, dtype=np.int64), np.asarray(leaf_ids, dtype=np.int64)
    good = (tid >= 0) & (tid < sizes.size)
    tid, lid = tid[good], lid[good]
    good = (lid >= 0) & (lid < sizes[tid])
    tid, lid = tid[good], lid[good]
    depth_of = depth(sizes, arity)
    assert sizes.size < 1 << 23 and (sizes.size == 0 or int(sizes.max()) <= 1 << 40)  # (tree, node) packs into one int64
    total, level = 0, 0
    while tid.size:
        level += 1
        alive = depth_of[tid] >= level  # the tree has a level `level`
        nodes = np.unique((tid[alive] << 40) | (lid[alive] // arity))
        total += nodes.size
        tid, lid = nodes >> 40, nodes & ((1 << 40) - 1)
    return total
