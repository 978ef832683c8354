"""The numpy model of the roots and openings of a grown tree against its EARLIER roots
(p252_merkle{4,2}_forest_ragged_anchor_openings_device_into; csrc/forest_anchor.hip) that its tests compare the call with.  An anchor is
a count c <= n of a tree now of n leaves.  With A = arity, f_l(c) = c // A^l and d_l(c) = f_l(c) % A, of the tree as it was at c leaves:
node j of level l is the stored node of the grown tree while j < f_l(c); node j == f_l(c) exists iff c % A^l != 0 and is the partial node
P_l(c) = H(the stored nodes [A f_l(c), f_{l-1}(c)) of level l - 1, then P_{l-1}(c) if it exists, then zeros); right of it there is nothing.
Everything here reads the GROWN tree's full build (leaves (>= n, 4), levels = its levels 1 .. bottom-up in one array) and never a rebuild
of the first c leaves: that rebuild is what the tests hold the model against.  The node hash comes in as `digest`: (w, arity, 4) children
-> (w, 4) digests.  No torch here, and nothing of the library."""
import numpy as np

from . import forestfrontier as FF
from . import forestwitness as FW
from . import treeshape as TS

BAD_DEPTH = FW.BAD_DEPTH


def lowest_digit(c, arity):
    """the lowest level whose digit of c is not zero (c >= 1)"""
    l = 0
    while c // arity ** l % arity == 0:
        l += 1
    return l


def old_digests(c, arity):
    """digests an anchor costs: depth(c) minus the lowest level whose digit of c is not zero; none when c is a power of the arity"""
    top = TS.depth(c, arity)
    return 0 if c == arity ** top else top - lowest_digit(c, arity)


def _level(leaves, levels, n, l, arity):
    """level l of the grown tree's build"""
    if l == 0:
        return leaves[:n]
    starts = TS.level_starts(n, arity)
    return levels[starts[l - 1]:starts[l]]


def partial_nodes(leaves, levels, n, c, arity, digest):
    """({l: P_l(c)}, digests computed) for 1 <= c <= n, from the grown tree's build: one chain from the lowest non-zero digit of c up to
    depth(c)"""
    leaves, levels = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(levels, dtype=np.uint64).reshape(-1, 4)
    assert 1 <= c <= n
    out, hashed = {}, 0
    for l in range(1, TS.depth(c, arity) + 1):
        if c % arity ** l == 0:
            continue
        lo, hi = arity * (c // arity ** l), c // arity ** (l - 1)
        kids = np.zeros((1, arity, 4), dtype=np.uint64)
        kids[0, :hi - lo] = _level(leaves, levels, n, l - 1, arity)[lo:hi]
        if l - 1 in out:
            kids[0, hi - lo] = out[l - 1]
        out[l] = np.asarray(digest(kids)).reshape(4)
        hashed += 1
    return out, hashed


def root_of(leaves, levels, n, c, arity, digest, partial=None):
    """the root the tree had at c leaves: P_depth(c)(c), or the stored node when c == A^depth(c) (c == 1: the leaf, reduced mod p)"""
    leaves, levels = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(levels, dtype=np.uint64).reshape(-1, 4)
    top = TS.depth(c, arity)
    if c == arity ** top:
        return FF.reduce_leaf(leaves[0]) if c == 1 else _level(leaves, levels, n, top, arity)[0].copy()
    P = partial_nodes(leaves, levels, n, c, arity, digest)[0] if partial is None else partial
    return P[top].copy()


def opening_of(leaves, levels, n, c, i, arity, stride, digest, partial=None):
    """(the opening of leaf i in the tree as it was at c leaves, how many of its siblings are partial nodes); i >= c, c == 0 or c > n: a
    bad one.  partial = partial_nodes(..)[0], for a caller that opens many leaves under one anchor."""
    if c == 0 or c > n or i >= c:
        return FW.Witness(arity, stride), 0
    leaves, levels = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(levels, dtype=np.uint64).reshape(-1, 4)
    P = partial_nodes(leaves, levels, n, c, arity, digest)[0] if partial is None else partial
    out = FW.Witness(arity, stride, leaves[i], depth=TS.depth(c, arity))
    assert out.depth <= stride
    used = 0
    for l in range(out.depth):
        level, f = _level(leaves, levels, n, l, arity), c // arity ** l
        node = i // arity ** l
        group = [x for x in range(node - node % arity, node - node % arity + arity) if x != node]
        for j, x in enumerate(group):
            if x < f:
                out.siblings[l, j] = level[x]
            elif x == f and c % arity ** l:
                out.siblings[l, j] = P[l]
                used += 1
        out.positions[l] = node % arity
    return out, used
