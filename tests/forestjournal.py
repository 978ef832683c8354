"""A numpy model of the journal of p252_merkle{4,2}_forest_ragged_update_journaled_device_into (csrc/forest_journal.hip): which (tree,
level, node) one call must journal, the host bound of their number, and a host reference of the swap on (flat leaves, per-tree
level arrays).  Plain Python sets and loops: nothing here shares code with the library."""
import numpy as np

from testsupport.treeshape import depth, level_starts, level_widths, levels_len

SIZE_MAX = 2 ** 64 - 1


def journal_entries(sizes, arity, tid, lid):
    """the set of (tree, level, node) one call with the updates (tid[i], lid[i]) must journal: every valid leaf (level 0) once and
    every ancestor of one, the tree's top included (it stands for the root).  sizes[t] = 0: a bad tree."""
    seen = set()
    for t, leaf in zip(np.asarray(tid).tolist(), np.asarray(lid).tolist()):
        if t < 0 or t >= len(sizes) or leaf < 0 or leaf >= sizes[t]:
            continue
        n, i, level = int(sizes[t]), int(leaf), 0
        seen.add((t, 0, i))
        while n > 1:
            n, i, level = (n + arity - 1) // arity, i // arity, level + 1
            seen.add((t, level, i))
    return seen


def journal_bound(n_leaves, n_trees, max_leaves, k, arity):
    """k + sum over l = 1 .. depth of min(k, n_leaves // arity^l + n_trees); 0 for a zero size; saturating at SIZE_MAX"""
    if 0 in (n_leaves, n_trees, max_leaves, k):
        return 0
    total = k
    for l in range(1, depth(min(max_leaves, n_leaves), arity) + 1):
        total += min(k, n_leaves // arity ** l + n_trees)
    return min(total, SIZE_MAX)


def ids_to_tuples(ids):
    """(n, 4) uint32 journal ids -> [(tree, level, node)] (level -1: a void id)"""
    ids = np.asarray(ids).view(np.uint32).reshape(-1, 4).astype(np.int64)
    return [(int(t), int(y) - 1, int(lo) | (int(hi) << 32)) for t, y, lo, hi in ids]


def split_levels(levels, sizes, arity):
    """the tree-major d_levels (used part) -> one writable (levels_len(n_t), 4) array per tree"""
    out, at = [], 0
    for n in sizes:
        ln = levels_len(n, arity)
        out.append(levels[at:at + ln].copy())
        at += ln
    return out


def swap_host(leaves, off, sizes, levels_per_tree, ids, values, n, arity, roots=None, reduce=None):
    """the first n entries of (ids, values) exchanged with the nodes they name, in place in leaves (flat, (N, 4) uint64),
    levels_per_tree and values; roots[t] follows an entry that is its tree's top (reduce = the map from a one-leaf tree's leaf to its
    root).  -> the number of entries that name no node of the forest (nothing written for them)"""
    bad = 0
    for g, (t, level, i) in enumerate(ids_to_tuples(ids)[:n]):
        if level < 0 or t >= len(sizes) or sizes[t] == 0:
            bad += 1
            continue
        counts = [int(sizes[t])] + level_widths(sizes[t], arity)  # nodes of level 0 (the leaves), 1, ..: the last one is 1
        if level >= len(counts) or i >= counts[level]:
            bad += 1
            continue
        if level == 0:
            row = leaves[int(off[t]) + i]
        else:
            row = levels_per_tree[t][level_starts(sizes[t], arity)[level - 1] + i]
        mine = values[g].copy()
        values[g] = row
        row[...] = mine
        if roots is not None and counts[level] == 1:
            roots[t] = reduce(mine) if (level == 0 and reduce is not None) else mine
    return bad
