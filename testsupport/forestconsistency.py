"""The numpy model of the consistency proofs of a ragged forest (p252_merkle{4,2}_forest_ragged_consistency_device_into and
_forest_consistency_verify_device_into; csrc/forest_consistency.hip) that their tests compare the calls with.  The proof that a tree of
m leaves is the tree it was at n < m leaves with leaves appended is the opening of leaf index n of the tree of m leaves
(forestwitness.opening_of): with A = arity, f_l(n) = n // A^l and d_l(n) = f_l(n) % A its slot on row l is d_l(n) and its siblings left
of the slot are the nodes [A f_{l+1}(n), f_l(n)) of level l — row l of forestfrontier.frontier_of at n.  Two independent things: the
proof cut out of a full build (proof_of) and its check (verify), whose old side is forestfrontier.root_of fed with the left siblings.
The node hash comes in as `digest`: (w, arity, 4) children -> (w, 4) digests.  No torch here, and nothing of the library."""
import numpy as np

from . import forestfrontier as FF
from . import forestwitness as FW
from . import treeshape as TS

BAD_DEPTH = FW.BAD_DEPTH


def digits(n, arity, rows):
    """d_l(n) for l = 0 .. rows - 1"""
    return np.array([n // arity ** l % arity for l in range(rows)], dtype=np.uint8)


def proof_of(leaves, levels, m, n, arity, stride):
    """(the proof, the new count) for old count n of a tree of m leaves, cut out of its full build (leaves (>= m, 4), levels = its levels
    1 .. bottom-up in one array; m == 0: a bad or unknown tree).  1 <= n < m: the opening of leaf n.  n == m: zeros with the depth of m.
    n == 0, n > m or m == 0: a bad one (all zero, depth 0xFF) and new count 0."""
    if m == 0 or n == 0 or n > m:
        return FW.Witness(arity, stride), 0
    if n == m:
        return FW.Witness(arity, stride, depth=TS.depth(m, arity)), m
    return FW.opening_of(leaves, levels, m, n, arity, stride), m


def left_rows(proof, n, arity):
    """the siblings left of the slots d_l(n), as frontier rows: (stride + 1, arity - 1, 4), row l holding the first d_l(n) siblings of
    row l of the proof and zeros"""
    rows = np.zeros((proof.stride + 1, arity - 1, 4), dtype=np.uint64)
    for l in range(proof.stride):
        d = n // arity ** l % arity
        rows[l, :d] = proof.siblings[l, :d]
    return rows


def old_digests(n, arity):
    """digests of the old chain: none when n == A^depth(n) (the root is a final node); otherwise one per level from the lowest
    non-zero digit of n up to depth(n) - 1"""
    top = TS.depth(n, arity)
    if n == arity ** top:
        return 0
    low = next(l for l in range(top) if n // arity ** l % arity)
    return top - low


def n_hashed(n, m, arity):
    """digests of one check: depth(m) for the new chain plus the old chain's; none when n == m (or the proof is refused)"""
    return TS.depth(m, arity) + old_digests(n, arity) if 1 <= n < m else 0


def roots_many(leaves, siblings, n, m, digest, arity):
    """verify's two chains for k proofs with 1 <= n[i] < m[i] at once, level by level, so that `digest` is called once per level and
    chain: leaves (k, 4), siblings (k, D, arity - 1, 4), n and m (k,) -> (old roots (k, 4), new roots (k, 4), digests computed).  The
    slots are the digits of n; nothing else of a proof is looked at (tests/test_forest_consistency_cpu.py ties it to verify)."""
    leaves, siblings = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4), np.asarray(siblings, dtype=np.uint64)
    n, m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
    k = leaves.shape[0]
    dn, dm = TS.depth(n, arity), TS.depth(m, arity)
    cur, carry, has = leaves.copy(), np.zeros((k, 4), dtype=np.uint64), np.zeros(k, dtype=bool)
    hashed, rows = 0, np.arange(k)
    for l in range(int(dm.max(initial=0))):
        d = n // arity ** l % arity
        need = (l < dn) & ((d > 0) | has)
        if need.any():
            kids = np.zeros((k, arity, 4), dtype=np.uint64)
            for s in range(arity - 1):
                kids[d > s, s] = siblings[d > s, l, s]
            kids[rows, d] = carry  # (zero where there is none)
            carry[need] = np.asarray(digest(np.ascontiguousarray(kids[need]))).reshape(-1, 4)
            has |= need
            hashed += int(need.sum())
        final = (l == dn) & ~has  # n == A^depth(n): the final node left of the path
        carry[final] = siblings[final, l, 0]
        live = l < dm
        kids = np.zeros((k, arity, 4), dtype=np.uint64)
        for s in range(arity - 1):
            kids[rows, s + (s >= d)] = siblings[:, l, s]
        kids[rows, d] = cur
        cur[live] = np.asarray(digest(np.ascontiguousarray(kids[live]))).reshape(-1, 4)
        hashed += int(live.sum())
    old = np.array([FF.reduce_leaf(c) for c in carry], dtype=np.uint64).reshape(k, 4)
    return old, cur, hashed


def verify(proof, n, old_root, m, new_root, digest, arity):
    """(verdict, the old root recomputed, the new root recomputed, digests computed).  Refused — not 1 <= n <= m, or a depth byte other
    than depth(m), or one above the stride: verdict 0, zero roots, nothing hashed.  n == m: the verdict is whether the two claimed
    roots are the same, the roots out are the claimed ones, nothing hashed.  n < m: the slots must be the digits of n; the new chain is
    the ordinary re-hash with the slots taken from n; the old chain is forestfrontier.root_of over the left siblings."""
    zero = np.zeros(4, dtype=np.uint64)
    old_root, new_root = np.asarray(old_root, dtype=np.uint64).reshape(4), np.asarray(new_root, dtype=np.uint64).reshape(4)
    if not 1 <= n <= m:
        return 0, zero, zero, 0
    top = TS.depth(m, arity)
    if proof.depth != top or top > proof.stride:
        return 0, zero, zero, 0
    if n == m:
        return int(np.array_equal(old_root, new_root)), old_root.copy(), new_root.copy(), 0
    calls = [0]

    def counted(kids):
        calls[0] += kids.shape[0]
        return digest(kids)
    slots = digits(n, arity, top)
    cur = proof.leaf
    for l in range(top):
        kids = np.insert(proof.siblings[l], int(slots[l]), cur, axis=0)
        cur = np.asarray(counted(kids.reshape(1, arity, 4))).reshape(4)
    # a final node that IS the old root (n == A^depth(n)) is reduced as the leaf of a one-leaf tree is; a node is canonical already
    old = FF.reduce_leaf(FF.root_of(FF.State(arity, 0, n, left_rows(proof, n, arity)), counted))
    ok = np.array_equal(proof.positions[:top], slots) and np.array_equal(cur, new_root) and np.array_equal(old, old_root)
    return int(ok), old, cur, calls[0]
