"""The geometry of a Merkle tree and of a tree-major forest of them, once: what every numpy model, test helper and bench tool that needs
the shape of a tree imports.  Pure Python and numpy, and nothing of the library: a model that asks the code under test is no reference
(tests/test_treeshape_cpu.py ties these functions to the ABI's p252_merkle{4,2}_depth and _levels_len in one place).

A tree of n leaves has levels 1, 2, .. above them, level l of ceil(n / arity^l) nodes, up to the level of one node; n <= 1 has none.  Its
block of a forest's tree-major levels holds them bottom-up, and tree t's block follows the blocks of the trees before it.  Every
function of a leaf count takes one count (-> Python ints) or an array of counts (-> int64 arrays, element by element)."""
import numpy as np


def _counts(n):
    return np.asarray(n, dtype=np.int64) if np.ndim(n) else int(n)


def level_widths(n, arity):
    """nodes of levels 1, 2, .. of a tree of n leaves (none for n <= 1); for an array of leaf counts one array per level of the deepest
    tree, 0 where a tree has no such level"""
    n, out = _counts(n), []
    top = n if isinstance(n, int) else int(n.max(initial=0))  # the deepest tree decides how many levels there are
    while top > 1:
        top = (top + arity - 1) // arity
        n = (n + arity - 1) // arity * (n > 1)
        out.append(n)
    return out


def depth(n, arity):
    """levels above the leaves (p252_merkle{4,2}_depth)"""
    return sum((w > 0 for w in level_widths(n, arity)), _counts(n) * 0)


def levels_len(n, arity):
    """nodes above the leaves: the length of the tree's block (p252_merkle{4,2}_levels_len)"""
    return sum(level_widths(n, arity), _counts(n) * 0)


def offsets(sizes, start=0, dtype=np.uint64):
    """len(sizes) + 1 prefix sums from `start`: leaf offsets from leaf counts, block starts from levels_len, add_offsets from appends"""
    off = np.zeros(len(sizes) + 1, dtype=dtype)
    np.cumsum(np.asarray(sizes, dtype=dtype), out=off[1:])
    return off + dtype(start)


def block_starts(sizes, arity, dtype=np.int64):
    """where every tree's block begins in a forest's tree-major levels: len(sizes) + 1 entries, the last the length in use"""
    return offsets(levels_len(sizes, arity), dtype=dtype)


def level_starts(n, arity):
    """where levels 1, 2, .. of ONE tree of n leaves begin inside its block; one more entry than levels, the last levels_len(n)"""
    starts = [0]
    for w in level_widths(int(n), arity):
        starts.append(starts[-1] + w)
    return starts


def levels_bound(n_leaves, n_trees, max_leaves, arity):
    """what the tree-major levels of any forest of n_trees trees, n_leaves leaves in all and none above max_leaves, fit in"""
    return n_leaves // (arity - 1) + n_trees * depth(max_leaves, arity)
