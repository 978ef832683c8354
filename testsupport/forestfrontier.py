"""The numpy model of a Merkle tree kept only as its frontier (p252_merkle{4,2}_forest_frontier_append_device_into and
_extract_device_into; csrc/forest_frontier.hip) that their tests compare the calls with.  With A = arity, f_l(n) = n // A^l, c_l(n) =
ceil(n / A^l) and d_l(n) = f_l(n) % A: row l of the frontier of a tree of n leaves holds the d_l(n) nodes [A f_{l+1}(n), f_l(n)) of
level l (level 0: the leaves), rows 0 .. D(max_leaves), the slots past d_l(n) zero.  Three independent things: the frontier cut out of
a full build (frontier_of), the frontier carried through an append (append), and the root recomputed from a frontier alone (root_of).
The node hash comes in as `digest`: (w, arity, 4) children -> (w, 4) digests (the tests pass the oracle's).  No torch here."""
import numpy as np

from . import treeshape as TS


class State:
    """one tree: arity, max_leaves, n (its leaves so far), rows (D + 1, arity - 1, 4) uint64, root (4,) uint64 (zero: empty)"""

    def __init__(self, arity, max_leaves, n=0, rows=None, root=None):
        self.arity, self.max_leaves, self.n = arity, max_leaves, n
        self.rows = np.zeros((rows_of(max_leaves, arity), arity - 1, 4), dtype=np.uint64) if rows is None else rows
        self.root = np.zeros(4, dtype=np.uint64) if root is None else root


def rows_of(max_leaves, arity):
    """rows of a frontier: D(max_leaves) + 1"""
    return TS.depth(max_leaves, arity) + 1


def bound(max_leaves, arity):
    """p252_merkle{4,2}_forest_frontier_bound"""
    return rows_of(max_leaves, arity) * (arity - 1) if max_leaves else 0


def n_hashed(n, m, arity):
    """digests of an append of m leaves to a tree of n: sum over l = 1 .. D(n + m) of c_l(n + m) - f_l(n); none for m == 0"""
    if m == 0:
        return 0
    return sum(-(-(n + m) // arity ** l) - n // arity ** l for l in range(1, TS.depth(n + m, arity) + 1))


def accepted_appends(counts, add_offsets, n_add, max_leaves):
    """the call's refusal rules -> (m per tree, 0 where refused; refused per tree): decreasing offsets, a range past n_add, a count
    above max_leaves (a corrupt state, whatever it is given), n + m > max_leaves, and the sum rule of the stored append — an append
    that takes the appends before it (those that passed the per-tree rules) past n_add"""
    aoff = [int(x) for x in np.asarray(add_offsets).reshape(-1)]
    m, refused, run = [], [], 0
    for t, n in enumerate(int(x) for x in np.asarray(counts).reshape(-1)):
        lo, hi = aoff[t], aoff[t + 1]
        mt = hi - lo
        ok = hi >= lo and hi <= n_add and n <= max_leaves and n + mt <= max_leaves
        mt = mt if ok else 0
        if ok and mt and (run > n_add or mt > n_add - run):
            ok = False
        run += mt
        m.append(mt if ok else 0)
        refused.append(not ok)
    return m, refused


def reduce_leaf(leaf):
    """the limbs mod p: the root of a one-leaf tree"""
    import oracle
    return oracle.int_to_limbs(oracle.limbs_to_int(leaf) % oracle.P)


def frontier_of(leaves, levels, n, arity, max_leaves):
    """the rows of a tree of n leaves, cut out of its full build: leaves (n, 4) and levels = its levels 1 .. bottom-up in one array
    (what the single-tree calls and the oracle write)"""
    leaves, levels = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(levels, dtype=np.uint64).reshape(-1, 4)
    rows = np.zeros((rows_of(max_leaves, arity), arity - 1, 4), dtype=np.uint64)
    starts = TS.level_starts(n, arity)
    for l in range(rows.shape[0]):
        lo, hi = arity * (n // arity ** (l + 1)), n // arity ** l
        if hi > lo:
            level = leaves[:n] if l == 0 else levels[starts[l - 1]:starts[l]]
            rows[l, :hi - lo] = level[lo:hi]
    return rows


def append(state, leaves, digest):
    """state with `leaves` (m, 4) appended -> (the new State, the digests computed); the argument is left as it is"""
    A, n = state.arity, state.n
    V = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4)
    m = V.shape[0]
    if m == 0:
        return State(A, state.max_leaves, n, state.rows.copy(), state.root.copy()), 0
    nn = n + m
    assert nn <= state.max_leaves
    rows, hashed, top = state.rows.copy(), 0, TS.depth(nn, A)
    for l in range(top + 1):
        f_old, f_new, up_old, up_new = n // A ** l, nn // A ** l, n // A ** (l + 1), nn // A ** (l + 1)
        # the new row l, from V_l alone
        if up_new == up_old:
            rows[l, f_old - A * up_old:f_new - A * up_old] = V[:f_new - f_old]
        else:
            d = f_new - A * up_new
            rows[l] = 0
            rows[l, :d] = V[A * up_new - f_old:A * up_new - f_old + d]
        if l == top:
            break
        # V_{l+1}: the nodes [f_{l+1}(n), c_{l+1}(n')) from the old row l and V_l
        d_old, width = f_old - A * up_old, -(-nn // A ** l)
        count = -(-nn // A ** (l + 1)) - up_old
        kids = np.zeros((count * A, 4), dtype=np.uint64)
        kids[:d_old] = state.rows[l, :d_old]
        have = width - A * up_old - d_old  # children that V_l holds
        assert have == V.shape[0]
        kids[d_old:d_old + have] = V
        V = np.asarray(digest(kids.reshape(count, A, 4))).reshape(count, 4)
        hashed += count
    root = reduce_leaf(V[0]) if nn == 1 else V[0].copy()
    return State(A, state.max_leaves, nn, rows, root), hashed


def root_of(state, digest):
    """the root from the frontier alone: the chain of partly filled nodes — at level l the final nodes of row l, then the partly
    filled node of level l (if n is no multiple of A^l), then zeros"""
    A, n = state.arity, state.n
    if n == 0:
        return np.zeros(4, dtype=np.uint64)
    top = TS.depth(n, A)
    if n == A ** top:  # the root is final: row D holds it (one leaf: reduced)
        return reduce_leaf(state.rows[0, 0]) if n == 1 else state.rows[top, 0].copy()
    carry = None
    for l in range(top):
        d = n // A ** l % A
        kids = [state.rows[l, k] for k in range(d)] + ([carry] if carry is not None else [])
        if not kids:
            carry = None
            continue
        block = np.zeros((1, A, 4), dtype=np.uint64)
        block[0, :len(kids)] = np.array(kids)
        carry = np.asarray(digest(block)).reshape(4)
    return carry
