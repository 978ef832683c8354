"""The numpy model of the openings of marked leaves kept current while a tree that is kept only as its frontier grows
(p252_merkle{4,2}_forest_frontier_append_witness_device_into; csrc/forest_witness.hip) that its tests compare the call with.  A witness
is an opening in the layout of p252_merkle{4,2}_forest_ragged_openings_device at a stride of D rows: the leaf, per row l < depth the
arity - 1 siblings of the path's node (its group's nodes in index order, its own left out) and its slot in the group, zero rows from the
depth on.  Two independent things: the opening cut out of a full build (opening_of), and the opening at count n carried through an
append of m leaves with nothing but the old frontier, the nodes the append computes and zeros (refresh).  Beside them, for the bench
tool: the bytes that rule reads and writes for a set of witnesses (pass_bytes).  With A = arity, f_l(n) =
n // A^l and c_l(n) = ceil(n / A^l) the append computes V_l = the nodes [f_l(n), c_l(n + m)) of level l, V_0 = the new leaves
(computed_levels: forestfrontier.append's own loop).  The node hash comes in as `digest`: (w, arity, 4) children -> (w, 4) digests.
No torch here."""
import numpy as np

from . import forestfrontier as FF
from . import treeshape as TS

BAD_DEPTH = 0xFF


class Witness:
    """leaf (4,) uint64, siblings (D, arity - 1, 4) uint64, positions (D,) uint8, depth (0xFF: a bad one, all zero)"""

    def __init__(self, arity, stride, leaf=None, siblings=None, positions=None, depth=BAD_DEPTH):
        self.leaf = np.zeros(4, dtype=np.uint64) if leaf is None else np.asarray(leaf, dtype=np.uint64).copy()
        self.siblings = np.zeros((stride, arity - 1, 4), dtype=np.uint64) if siblings is None else np.asarray(siblings, dtype=np.uint64).copy()
        self.positions = np.zeros(stride, dtype=np.uint8) if positions is None else np.asarray(positions, dtype=np.uint8).copy()
        self.depth = int(depth)
        self.arity, self.stride = arity, stride

    def copy(self):
        return Witness(self.arity, self.stride, self.leaf, self.siblings, self.positions, self.depth)

    def bad(self):
        return self.depth == BAD_DEPTH

    def __eq__(self, other):
        return (self.depth == other.depth and np.array_equal(self.leaf, other.leaf) and np.array_equal(self.siblings, other.siblings)
                and np.array_equal(self.positions, other.positions))


def opening_of(leaves, levels, n, p, arity, stride):
    """the opening of leaf p of a tree of n leaves, cut out of its full build: leaves (>= n, 4) and levels = its levels 1 .. bottom-up
    in one array (what the single-tree calls and the oracle write); p >= n: a bad one"""
    if p >= n:
        return Witness(arity, stride)
    leaves, levels = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(levels, dtype=np.uint64).reshape(-1, 4)
    starts = TS.level_starts(n, arity)
    out = Witness(arity, stride, leaves[p], depth=TS.depth(n, arity))
    assert out.depth <= stride
    for l in range(out.depth):
        level = leaves[:n] if l == 0 else levels[starts[l - 1]:starts[l]]
        node = p // arity ** l
        group = [x for x in range(node - node % arity, node - node % arity + arity) if x != node]
        for j, x in enumerate(group):
            if x < level.shape[0]:
                out.siblings[l, j] = level[x]
        out.positions[l] = node % arity
    return out


def computed_levels(state, leaves, digest):
    """[V_0, V_1, .. V_D(n + m)] of an append of `leaves` (m > 0, 4) to `state` (a forestfrontier.State), V_l = the nodes
    [f_l(n), c_l(n + m)) — from the old rows and the level below, as forestfrontier.append computes them"""
    A, n = state.arity, state.n
    V = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4)
    nn = n + V.shape[0]
    out = [V]
    for l in range(TS.depth(nn, A)):
        f_old, up_old = n // A ** l, n // A ** (l + 1)
        d_old, count = f_old - A * up_old, -(-nn // A ** (l + 1)) - up_old
        kids = np.zeros((count * A, 4), dtype=np.uint64)
        kids[:d_old] = state.rows[l, :d_old]
        kids[d_old:d_old + V.shape[0]] = V
        V = np.asarray(digest(kids.reshape(count, A, 4))).reshape(count, 4)
        out.append(V)
    return out


def refresh(witness, p, state_old, new_leaves, digest, computed=None):
    """the witness of leaf p after `new_leaves` (m, 4) were appended to `state_old` (a forestfrontier.State of n leaves); the argument is
    left as it is.  p >= n + m: bad.  p < n: `witness` must be the opening at n — a depth byte other than depth(n) makes it bad when
    the tree grows, and m == 0 leaves it as it is, whatever it holds.  n <= p < n + m: the input is ignored.  computed =
    computed_levels(state_old, new_leaves, digest), for a caller that refreshes many witnesses of one append."""
    A, n, D = state_old.arity, state_old.n, witness.stride
    new_leaves = np.asarray(new_leaves, dtype=np.uint64).reshape(-1, 4)
    nn = n + new_leaves.shape[0]
    if p >= nn:
        return Witness(A, D)
    if p < n and nn == n:
        return witness.copy()
    if p < n and witness.depth != TS.depth(n, A):
        return Witness(A, D)
    V = computed_levels(state_old, new_leaves, digest) if computed is None else computed
    top = TS.depth(nn, A)
    out = witness.copy() if p < n else Witness(A, D, new_leaves[p - n])
    for l in range(top):
        node, f, c = p // A ** l, n // A ** l, -(-nn // A ** l)
        group = [x for x in range(node - node % A, node - node % A + A) if x != node]
        for j, x in enumerate(group):
            if x < f:  # final: in the witness already, or — for a leaf this append brings — in the old row l
                if p >= n:
                    out.siblings[l, j] = state_old.rows[l, x - A * (n // A ** (l + 1))]
            elif x < c:
                out.siblings[l, j] = V[l][x - f]
            else:
                out.siblings[l, j] = 0
        out.positions[l] = node % A
    out.depth = top
    return out


def pass_bytes(arity, D, sizes, adds, tid, lid):
    """(read, written) bytes of the witnesses' pass, from the rule: per (witness, row) lane the ids, the depth byte and the tree's two
    words are read; a written row stores its position byte and every sibling that is not final, and reads those it copies"""
    la = 2 if arity == 4 else 1
    sizes, adds = np.asarray(sizes, dtype=np.int64), np.asarray(adds, dtype=np.int64)
    n, m, p = sizes[tid], adds[tid], np.asarray(lid, dtype=np.int64)
    nn = n + m
    top = TS.depth(nn, arity)
    lanes = len(tid) * max(D, 1)
    read, written = lanes * (4 + 8 + 1 + 16), 0
    grown = m > 0
    for l in range(D):
        live = grown & (l < top)
        node, f, c = p >> (l * la), n >> (l * la), -(-nn >> (l * la))
        carried = p < n
        row = live & ~(carried & ((p >> ((l + 1) * la)) < (n >> ((l + 1) * la))))
        first = node - (node & (arity - 1))
        for s in range(arity):
            x = first + s
            sib = row & (x != node)
            copied = sib & ((x >= f) | ~carried) & (x < c)
            zeroed = sib & (x >= c)
            read += int(copied.sum()) * 32
            written += int((copied | zeroed).sum()) * 32
        written += int(row.sum())
        fresh = grown & ~carried & (l >= top)  # a new witness's rows above its depth: zeroed
        written += int(fresh.sum()) * ((arity - 1) * 32 + 1)
    new = grown & (p >= n)
    return read + int(new.sum()) * 32, written + int(new.sum()) * 32 + int(grown.sum())
