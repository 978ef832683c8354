"""The model of the forest select (p252_merkle{4,2}_forest_ragged_select_device_into) that its tests compare the call with: which
picks are refused, where every picked tree lands, and the numpy gather that turns the sources' own arrays into the expected leaves,
levels and roots.  No torch here: the CPU tests import it too."""
import numpy as np

from testsupport.treeshape import block_starts, levels_len


def select_model(arity, sizes_a, bad_a, sizes_b, bad_b, pick, leaves_cap):
    """sizes_x: the leaf counts of the source's trees as its offsets give them, bad_x: the trees its build calls bad (empty ones
    are bad whether listed or not).  -> dict: per pick `source` (0: A, 1: B, -1: none), `tree`, `n` (the leaf count it brings, 0 when
    refused), `refused`; `offsets_new` and `level_starts` (n_pick + 1 each) and `n_bad`"""
    sizes_a, sizes_b = [int(s) for s in sizes_a], [int(s) for s in sizes_b]
    bad_a, bad_b = set(bad_a) | {t for t, s in enumerate(sizes_a) if s == 0}, set(bad_b) | {t for t, s in enumerate(sizes_b) if s == 0}
    source, tree, n, refused = [], [], [], []
    run = 0  # the sum of s_j, refused picks of good trees included: once past the cap, every later non-empty pick is refused
    for ident in pick:
        ident = int(ident)
        if ident < len(sizes_a):
            src, t, s = 0, ident, 0 if ident in bad_a else sizes_a[ident]
        elif ident - len(sizes_a) < len(sizes_b):
            src, t = 1, ident - len(sizes_a)
            s = 0 if t in bad_b else sizes_b[t]
        else:
            src, t, s = -1, -1, 0
        run += s
        ok = s > 0 and run <= leaves_cap
        source.append(src), tree.append(t), n.append(s if ok else 0), refused.append(not ok)
    offsets_new = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    level_starts = block_starts(n, arity, dtype=np.uint64)
    return dict(source=source, tree=tree, n=n, refused=refused, offsets_new=offsets_new, level_starts=level_starts, n_bad=sum(refused))


def gather(model, arity, forest_a, forest_b=None):
    """forest_x = (leaves (n, 4), offsets, level_starts, levels (m, 4), roots (n_trees, 4)) as numpy arrays, level_starts = the prefix
    sums of levels_len over the source's GOOD trees' sizes (a bad tree has no block) -> the expected (leaves, levels, roots) of the new
    forest, exact-sized"""
    leaves, levels, roots = [], [], []
    for src, t, n, refused in zip(model["source"], model["tree"], model["n"], model["refused"]):
        if refused:
            roots.append(np.zeros((1, 4), np.uint64))
            continue
        f_leaves, f_off, f_lo, f_levels, f_roots = forest_a if src == 0 else forest_b
        lo, ll = int(f_off[t]), int(f_lo[t])
        leaves.append(f_leaves[lo:lo + n])
        levels.append(f_levels[ll:ll + levels_len(n, arity)])
        roots.append(f_roots[t:t + 1])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros((0, 4), np.uint64)  # noqa: E731
    return cat(leaves), cat(levels), cat(roots)


def level_starts_of(sizes, bad, arity):
    """the block starts of a source forest's tree-major levels: the prefix sums of levels_len over its trees, bad ones counting 0"""
    bad = set(bad)
    return block_starts([0 if t in bad else s for t, s in enumerate(sizes)], arity, dtype=np.uint64)
