"""The numpy models of the append (p252_merkle{4,2}_forest_ragged_append_device_into) and of the resize
(p252_merkle{4,2}_forest_ragged_resize_device_into) that their tests compare the calls with: which trees and appends are refused, where
every leaf and node of the new forest comes from, and which nodes are hashed.  Two models on purpose: the tests check one against the
other (keep None, no tree dropped).  No torch here: the CPU tests import it too."""
import numpy as np

from .treeshape import level_widths

KEEP_ALL = (1 << 64) - 1


def good_leaf_counts(offsets, n_leaves, max_leaves):
    """the build's validation of a forest (k_fr_prep and the sum rule): n_t, or 0 for a bad tree"""
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    out, run = [], 0
    for t in range(len(off) - 1):
        lo, hi = off[t], off[t + 1]
        n = hi - lo
        n = n if (hi >= lo and 1 <= n <= max_leaves and hi <= n_leaves) else 0
        if run > n_leaves or n > n_leaves - run:
            run, n = run + n, 0
        else:
            run += n
        out.append(n)
    return out


def forest_append_model(offsets, n_leaves, max_leaves, add_offsets, n_add, max_leaves_new, arity):
    """What p252_merkle{4,2}_forest_ragged_append_device_into does to a forest (offsets: n_trees + 1, or empty for no old forest) given
    add_offsets (n_trees_new + 1).  Returns a dict:
      n_old, m, refused   per tree of the new forest: the old leaf count (the build's validation), the accepted append, its refusal
      offsets_new         n_trees_new + 1
      leaf_src            per new leaf: its index in the old leaves, or -1 - (its index in d_add)
      lo_new, lo_old      block starts of the tree-major levels, n_trees_new + 1 / n_trees + 1
      node_src            per used slot of the new levels: the slot of the old levels it is moved from, or -1 (dirty: hashed)
      node_id             per used slot: (tree, level, index)
      dirty               {level: [(tree, index), ..]} in the order of the call's lists
      n_hashed, n_bad"""
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    aoff = [int(x) for x in np.asarray(add_offsets).reshape(-1)]
    T = len(aoff) - 1
    old = good_leaf_counts(off, n_leaves, max_leaves) if len(off) > 1 else []
    n_old = [old[t] if t < len(old) else 0 for t in range(T)]
    m, refused, run = [], [], 0
    for t in range(T):
        lo, hi = aoff[t], aoff[t + 1]
        mt = hi - lo
        ok = hi >= lo and hi <= n_add and n_old[t] + mt <= max_leaves_new
        mt = mt if ok else 0
        if ok and mt and (run > n_add or mt > n_add - run):  # the sum rule: overlapping ranges behind decreasing offsets
            ok = False
        run += mt
        m.append(mt if ok else 0)
        refused.append(not ok)
    n_new = [a + b for a, b in zip(n_old, m)]
    offsets_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(n_new, out=offsets_new[1:])
    leaf_src = np.empty(int(offsets_new[-1]), dtype=np.int64)
    for t in range(T):
        at = int(offsets_new[t])
        if n_old[t]:
            leaf_src[at:at + n_old[t]] = off[t] + np.arange(n_old[t])
        if m[t]:
            leaf_src[at + n_old[t]:at + n_new[t]] = -1 - (aoff[t] + np.arange(m[t]))
    lo_old = np.zeros(len(old) + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in old], out=lo_old[1:])
    lo_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in n_new], out=lo_new[1:])
    node_src = np.full(int(lo_new[-1]), -1, dtype=np.int64)
    node_id = []
    dirty, n_hashed = {}, 0
    for t in range(T):
        w_new, w_old = level_widths(n_new[t], arity), level_widths(n_old[t], arity)
        start_new, start_old = int(lo_new[t]), int(lo_old[t]) if t < len(old) else 0
        for l, w in enumerate(w_new, 1):
            clean = w if m[t] == 0 else n_old[t] // arity ** l
            node_src[start_new:start_new + clean] = start_old + np.arange(clean)
            node_id += [(t, l, j) for j in range(w)]
            if w > clean:
                dirty.setdefault(l, []).extend((t, j) for j in range(clean, w))
                n_hashed += w - clean
            start_new += w
            if l <= len(w_old):
                start_old += w_old[l - 1]
    n_bad = sum(1 for t in range(T) if refused[t] or n_new[t] == 0)
    return {"n_old": n_old, "m": m, "refused": refused, "n_new": n_new, "offsets_new": offsets_new, "leaf_src": leaf_src, "lo_new": lo_new,
            "lo_old": lo_old, "node_src": node_src, "node_id": node_id, "dirty": dirty, "n_hashed": n_hashed, "n_bad": n_bad}


def model_leaves(model, leaves, add):
    """the new forest's leaves (numpy (n, 4)) from the old ones and d_add"""
    src = model["leaf_src"]
    leaves, add = np.asarray(leaves).reshape(-1, 4), np.asarray(add).reshape(-1, 4)
    out = np.empty((src.size, 4), dtype=leaves.dtype if leaves.size else add.dtype)
    old = src >= 0
    out[old] = leaves[src[old]]
    out[~old] = add[-1 - src[~old]]
    return out


def forest_resize_model(offsets, n_leaves, max_leaves, keep, add_offsets, n_add, max_leaves_new, arity):
    """What p252_merkle{4,2}_forest_ragged_resize_device_into does to a forest (offsets: n_trees + 1, or empty for no old forest) given
    keep (n_trees_new values, or None: every tree whole) and add_offsets (n_trees_new + 1).  Returns forest_append_model's dict — with
    keep None and no tree dropped, the same values — plus
      k                   per tree of the new forest: the old leaves it keeps, min(keep[t], n_old[t])
    leaf_src / node_src name slots of the OLD forest's leaves / levels, or -1 - (index in d_add) / -1 (dirty: hashed).  A node of the
    new tree is clean iff its index is below floor(k / arity^level) — or the tree is unchanged (k == n_old, m == 0), whose last,
    partly filled parents are clean as well."""
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    aoff = [int(x) for x in np.asarray(add_offsets).reshape(-1)]
    T = len(aoff) - 1
    old = good_leaf_counts(off, n_leaves, max_leaves) if len(off) > 1 else []
    n_old = [old[t] if t < len(old) else 0 for t in range(T)]
    if keep is not None:  # (as uint64, one by one: a list that mixes 2^64 - 1 with small values would become floats in numpy)
        keep = [int(x) & KEEP_ALL for x in (keep.reshape(-1).tolist() if isinstance(keep, np.ndarray) else keep)]
        assert len(keep) == T
    k = list(n_old) if keep is None else [min(x, n) for x, n in zip(keep, n_old)]
    m, refused, run = [], [], 0
    for t in range(T):
        lo, hi = aoff[t], aoff[t + 1]
        mt = hi - lo
        ok = hi >= lo and hi <= n_add and k[t] + mt <= max_leaves_new
        mt = mt if ok else 0
        if ok and mt and (run > n_add or mt > n_add - run):  # the sum rule: overlapping ranges behind decreasing offsets
            ok = False
        run += mt
        m.append(mt if ok else 0)
        refused.append(not ok)
    n_new = [a + b for a, b in zip(k, m)]
    offsets_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(n_new, out=offsets_new[1:])
    leaf_src = np.empty(int(offsets_new[-1]), dtype=np.int64)
    for t in range(T):
        at = int(offsets_new[t])
        if k[t]:
            leaf_src[at:at + k[t]] = off[t] + np.arange(k[t])
        if m[t]:
            leaf_src[at + k[t]:at + n_new[t]] = -1 - (aoff[t] + np.arange(m[t]))
    lo_old = np.zeros(len(old) + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in old], out=lo_old[1:])
    lo_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in n_new], out=lo_new[1:])
    node_src = np.full(int(lo_new[-1]), -1, dtype=np.int64)
    node_id = []
    dirty, n_hashed = {}, 0
    for t in range(T):
        w_new, w_old = level_widths(n_new[t], arity), level_widths(n_old[t], arity)
        start_new, start_old = int(lo_new[t]), int(lo_old[t]) if t < len(old) else 0
        unchanged = m[t] == 0 and k[t] == n_old[t]
        for l, w in enumerate(w_new, 1):
            clean = w if unchanged else k[t] // arity ** l
            node_src[start_new:start_new + clean] = start_old + np.arange(clean)
            node_id += [(t, l, j) for j in range(w)]
            if w > clean:
                dirty.setdefault(l, []).extend((t, j) for j in range(clean, w))
                n_hashed += w - clean
            start_new += w
            if l <= len(w_old):
                start_old += w_old[l - 1]
    n_bad = sum(1 for t in range(T) if refused[t] or n_new[t] == 0)
    return {"n_old": n_old, "k": k, "m": m, "refused": refused, "n_new": n_new, "offsets_new": offsets_new, "leaf_src": leaf_src, "lo_new": lo_new,
            "lo_old": lo_old, "node_src": node_src, "node_id": node_id, "dirty": dirty, "n_hashed": n_hashed, "n_bad": n_bad}
