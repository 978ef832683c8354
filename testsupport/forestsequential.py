"""The numpy model of leaf updates of a ragged forest applied IN ORDER, each with its witness
(p252_merkle{4,2}_forest_ragged_update_sequential_device_into; csrc/forest_sequential.hip), twice: `sequential_model` applies the
updates one by one to host trees and records everything the call returns — the reference —, and `level_parallel_model` mirrors the
device's method: the list of the updates kept sorted by (tree, node, time), the as-of lookup by binary search, the merge rank.  Pure
numpy and nothing of the library; the node hash is the caller's digest((m, arity, 4)) -> (m, 4), and reduce((m, 4)) -> (m, 4) is the
leaf mod p of a one-leaf tree."""
import bisect

import numpy as np

from . import treeshape as TS

BAD_DEPTH = 0xFF


def stable_order(tree_ids, leaf_ids):
    """the indices sorted by (tree id, leaf id, index): what the call takes as d_order"""
    t, j = np.asarray(tree_ids, dtype=np.uint64), np.asarray(leaf_ids, dtype=np.uint64)
    return np.lexsort((np.arange(t.size), j, t)).astype(np.uint32)


def order_is_valid(order, tree_ids, leaf_ids):
    """every entry < k and (tree id, leaf id, index) strictly ascending along the order (which makes it a permutation)"""
    k = len(tree_ids)
    o = [int(x) for x in order]
    if len(o) != k or any(x >= k for x in o):
        return False
    keys = [(int(tree_ids[x]), int(leaf_ids[x]), x) for x in o]
    return all(a < b for a, b in zip(keys, keys[1:]))


def good_updates(sizes, tree_ids, leaf_ids):
    """update i is good iff its tree is known and not empty and the leaf is inside it (sizes: the trees' leaf counts, 0 for a bad tree)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.array([int(t) < sizes.size and 0 <= int(j) < int(sizes[int(t)]) for t, j in zip(tree_ids, leaf_ids)], dtype=bool)


def build_tree(leaves, arity, digest):
    """[leaves, level 1, .., the root's level] of one tree (levels zero-padded to a multiple of the arity; one leaf: the leaves alone)"""
    rows = [np.array(leaves, dtype=np.uint64).reshape(-1, 4)]
    while rows[-1].shape[0] > 1:
        n = rows[-1].shape[0]
        kids = np.zeros(((n + arity - 1) // arity * arity, 4), dtype=np.uint64)
        kids[:n] = rows[-1]
        rows.append(np.asarray(digest(kids.reshape(-1, arity, 4)), dtype=np.uint64).reshape(-1, 4))
    return rows


def build_forest(leaves, sizes, arity, digest):
    """the trees of a forest, each as build_tree gives it (an empty tree: None)"""
    off = TS.offsets(sizes, dtype=np.int64)
    return [build_tree(leaves[off[t]:off[t + 1]], arity, digest) if sizes[t] else None for t in range(len(sizes))]


def forest_arrays(trees, reduce):
    """(leaves, compact tree-major levels, roots) of such trees: what a fresh build of the leaves stores (an empty tree: a zero root)"""
    leaves = [t[0] for t in trees if t is not None]
    levels = [row for t in trees if t is not None for row in t[1:]]
    roots = [np.zeros(4, dtype=np.uint64) if t is None else (t[-1][0] if len(t) > 1 else np.asarray(reduce(t[0][:1])).reshape(4)) for t in trees]
    cat = lambda rows: np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.uint64)  # noqa: E731
    return cat(leaves), cat(levels), np.stack(roots)


class Witnesses:
    """what the call returns for k updates at stride D: sentinel-free arrays, the rows of bad updates zero"""

    def __init__(self, k, D, arity):
        self.old = np.zeros((k, 4), dtype=np.uint64)
        self.sib = np.zeros((k, D, arity - 1, 4), dtype=np.uint64)
        self.pos = np.zeros((k, D), dtype=np.uint8)
        self.dep = np.full(k, BAD_DEPTH, dtype=np.uint8)
        self.before = np.zeros((k, 4), dtype=np.uint64)
        self.after = np.zeros((k, 4), dtype=np.uint64)
        self.n_bad, self.n_hashed, self.touched = 0, 0, set()

    def same(self, other):
        return all(np.array_equal(getattr(self, n), getattr(other, n)) for n in ("old", "sib", "pos", "dep", "before", "after")) and \
            (self.n_bad, self.n_hashed, self.touched) == (other.n_bad, other.n_hashed, other.touched)


def _root(tree, reduce):
    return tree[-1][0].copy() if len(tree) > 1 else np.asarray(reduce(tree[0][:1]), dtype=np.uint64).reshape(4)


def sequential_model(trees, tree_ids, leaf_ids, new_leaves, max_leaves, arity, digest, reduce):
    """applies the updates one by one, IN PLACE on `trees` (build_forest's) -> Witnesses; digest is called once per update and level"""
    k, D = len(tree_ids), int(TS.depth(max_leaves, arity))
    sizes = [0 if t is None else t[0].shape[0] for t in trees]
    good = good_updates(sizes, tree_ids, leaf_ids)
    W = Witnesses(k, D, arity)
    for i in range(k):
        if not good[i]:
            W.n_bad += 1
            continue
        t, c = int(tree_ids[i]), int(leaf_ids[i])
        tree = trees[t]
        d = len(tree) - 1
        W.dep[i], W.old[i], W.before[i] = d, tree[0][c], _root(tree, reduce)
        tree[0][c] = new_leaves[i]
        for l in range(d):
            base, p = c - c % arity, c % arity
            kids = np.zeros((arity, 4), dtype=np.uint64)
            width = tree[l].shape[0]
            kids[:min(arity, width - base)] = tree[l][base:base + arity]
            W.pos[i, l] = p
            W.sib[i, l] = np.delete(kids, p, axis=0)
            c //= arity
            tree[l + 1][c] = np.asarray(digest(kids.reshape(1, arity, 4)), dtype=np.uint64).reshape(4)
        W.after[i] = _root(tree, reduce)
        W.n_hashed += d
        W.touched.add(t)
    return W


def level_parallel_model(trees, tree_ids, leaf_ids, new_leaves, order, max_leaves, arity, digest, reduce):
    """the device's method on the same inputs, IN PLACE on `trees` -> Witnesses.  Per level the list `keys` holds (tree, node, time) of
    every live element in ascending order with its value; a sibling as of time i is the value of the last element of its run before
    (tree, sibling, i), or the stored node; the parents' list is filled by the merge rank, and one digest call hashes the whole level."""
    k, D = len(tree_ids), int(TS.depth(max_leaves, arity))
    sizes = [0 if t is None else t[0].shape[0] for t in trees]
    good = good_updates(sizes, tree_ids, leaf_ids)
    W = Witnesses(k, D, arity)
    W.n_bad = int((~good).sum())
    # the list of level 0: the order's good entries
    keys = [(int(tree_ids[i]), int(leaf_ids[i]), int(i)) for i in order if good[i]]
    assert keys == sorted(keys)
    vals = [np.array(new_leaves[i], dtype=np.uint64) for _, _, i in keys]
    depth = lambda t: len(trees[t]) - 1  # noqa: E731
    for p, (t, c, i) in enumerate(keys):  # the heads of the witnesses
        W.dep[i] = depth(t)
        W.old[i] = vals[p - 1] if p and keys[p - 1][:2] == (t, c) else trees[t][0][c]
        W.n_hashed += depth(t)
        W.touched.add(t)
        if depth(t) == 0:
            W.before[i], W.after[i] = np.asarray(reduce(W.old[i:i + 1])).reshape(4), np.asarray(reduce(vals[p].reshape(1, 4))).reshape(4)
    for l in range(D + 1):
        live = [p for p, (t, _, _) in enumerate(keys) if l < depth(t)]
        children = np.zeros((len(live), arity, 4), dtype=np.uint64)
        ranks = []
        for row, p in enumerate(live):
            t, c, i = keys[p]
            own, width = c % arity, trees[t][l].shape[0]
            start, earlier, latest = None, 0, None
            for j in range(arity):
                n = c - own + j
                e = bisect.bisect_left(keys, (t, n, i))  # the first key >= (t, n, i): p itself for the own slot
                s = bisect.bisect_left(keys, (t, n, 0))
                if j == 0:
                    start = s
                earlier += e - s
                if e > s and (latest is None or keys[e - 1][2] > keys[latest][2]):
                    latest = e - 1
                if j == own:
                    assert e == p
                    children[row, j] = vals[p]
                elif n < width:
                    children[row, j] = vals[e - 1] if e > s else trees[t][l][n]
            W.pos[i, l] = own
            W.sib[i, l] = np.delete(children[row], own, axis=0)
            ranks.append((start + earlier, latest))
        # the write-back of level l, after every lookup of the level: the last element of a run holds the node's final value
        for p, (t, c, i) in enumerate(keys):
            if l <= depth(t) and (p + 1 == len(keys) or keys[p + 1][:2] != (t, c)):
                trees[t][l][c] = vals[p]
        if not live:
            break
        parents = np.asarray(digest(children), dtype=np.uint64).reshape(-1, 4)
        up_keys, up_vals = list(keys), list(vals)  # (the elements of trees that ended keep their place)
        row_of = {p: row for row, p in enumerate(live)}
        for row, p in enumerate(live):
            t, c, i = keys[p]
            q, latest = ranks[row]
            up_keys[q], up_vals[q] = (t, c // arity, i), parents[row]
            if depth(t) == l + 1:  # the parent is the root: before update i it was the parent's value of the latest earlier element
                W.after[i] = parents[row]
                W.before[i] = parents[row_of[latest]] if latest is not None else trees[t][l + 1][0]
        # the dead elements must not stand between live ones of their own tree: a tree's elements all end on the same level
        keys, vals = up_keys, up_vals
        assert [x for x in keys if l + 1 <= depth(x[0])] == sorted(x for x in keys if l + 1 <= depth(x[0]))
    return W
