"""Shapes that drive every two-level scan of the ragged calls past one block of tiles, the host-side expectations and the runners that
tests/test_scan_width_cpu.py (the shapes' conditions, on the numpy models alone) and tests/test_scan_width_gpu.py (the library) share.
A plain helper module, imported as forestwalk and edgecases are; no torch at module level.

Five kernels scan tile sums in a loop of one block per trip with a carry from trip to trip (k_fr_scan_tiles, k_fa_scan_tiles,
k_mp_scan_tiles, k_fm_scan_tiles, k_fm_tree_scan; the three over trees through one routine, scan_tile_row of csrc/blockops.hpp, with
each kernel's own block constant).  The tile and block constants are read out of the csrc text, the shapes are derived
from them, and the CPU test asserts on the models' counts that every shape makes the trips it is here for: a changed constant moves
the shapes or fails that test.

  constants()             the constexpr unsigned values of csrc
  wide_forest(arity)      2 trips + 3 tiles + 5 trees of 1 .. 2 * arity + 1 leaves
  expected_forest(..)     roots and tree-major levels by size class through any batch digest (none of the forest's scans)
  resize_counts(..)       forest_resize_model's n_new / n_hashed / n_bad, vectorised (held to it on a small forest)
  forest_multiproof_fast  forest_multiproof_extract / _counts, vectorised (held to them on a small forest)
  dense / sparse          positions of the single trees; fm_wide / fm_long_run / fm_aligned: the forest multiproof cases
  ragged_batch(n)         messages around the first octave bucket of the ragged hash's schedule
  run_*                   the call sequences on a Context; `python tests/scanwidth.py child ...` runs two of them in a fresh process"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
if ROOT not in sys.path:  # (a child process starts from this file alone: tests/ is its path already)
    sys.path.insert(0, ROOT)

import edgecases as E  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402

NAMES = ("FR_BLOCK", "FR_ITEMS", "FOREST_APPEND_SCAN_TILE", "FA_BLOCK", "MP_BLOCK", "FM_BLOCK", "FM_TREE_ITEMS", "RAGGED_EXACT_BLOCKS")
ARITIES = (4, 2)
SENTINEL = -0x0123456789ABCDEF
SENT64 = np.uint64(SENTINEL & E.M64)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def constants(csrc=CSRC):
    """{name: value} of every `constexpr unsigned NAME = <digits>;` line of csrc; the eight names the shapes hang on must be there"""
    out = {}
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".h", ".hpp", ".hip", ".cpp")):
            continue
        with open(os.path.join(csrc, name)) as fh:
            for m in re.finditer(r"^\s*constexpr unsigned\s+(\w+)\s*=\s*(\d+)u?\s*;", fh.read(), re.M):
                out[m.group(1)] = int(m.group(2))
    missing = [n for n in NAMES if n not in out]
    assert not missing, "csrc no longer defines %s as plain constexpr unsigned values" % missing
    return out


C = constants()
# kernel -> (elements of one tile, tiles of one trip of the loop)
SCANS = {
    "k_fr_scan_tiles": (C["FR_BLOCK"] * C["FR_ITEMS"], C["FR_BLOCK"]),
    "k_fa_scan_tiles": (C["FOREST_APPEND_SCAN_TILE"], C["FA_BLOCK"]),
    "k_mp_scan_tiles": (C["MP_BLOCK"], C["MP_BLOCK"]),
    "k_fm_scan_tiles": (C["FM_BLOCK"], C["FM_BLOCK"]),
    "k_fm_tree_scan": (C["FM_BLOCK"] * C["FM_TREE_ITEMS"], C["FM_BLOCK"]),
}
TREE_KERNELS = ("k_fr_scan_tiles", "k_fa_scan_tiles", "k_fm_tree_scan")


def chunk(kernel):
    """elements one trip of the kernel's loop covers"""
    tile, per_trip = SCANS[kernel]
    return tile * per_trip


def tiles(kernel, n):
    return -(-int(n) // SCANS[kernel][0])


def trips(kernel, n):
    return -(-tiles(kernel, n) // SCANS[kernel][1])


TREE_TILE = max(SCANS[k][0] for k in TREE_KERNELS)
TREE_CHUNK = max(chunk(k) for k in TREE_KERNELS)
LIST_CHUNK = max(chunk("k_mp_scan_tiles"), chunk("k_fm_scan_tiles"))
WIDE_TREES = 2 * TREE_CHUNK + 3 * TREE_TILE + 5


def leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60)"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(int(n), 4), dtype=np.uint64)


def trip_borders(n_trees):
    """the trees on both sides of every tile border next to a trip border (the border itself, one tile before, one tile after)"""
    out = []
    for c in range(TREE_CHUNK, n_trees, TREE_CHUNK):
        for b in (c - TREE_TILE, c, c + TREE_TILE):
            out += [t for t in (b - 1, b) if 0 <= t < n_trees]
    return sorted(set(out))


def at_trip_borders(n_trees):
    """the two trees on each side of every trip border"""
    return [t for c in range(TREE_CHUNK, n_trees, TREE_CHUNK) for t in (c - 1, c)]


# ---------------------------------------------------------------------------------------------- the wide forest
class WideForest:
    """sizes (T,), off (T + 1,), flat (n, 4), max_leaves, unreduced (the one-leaf trees whose leaf has limbs >= p), oracle_ids"""


def wide_forest(arity, n_trees=None):
    n_trees = WIDE_TREES if n_trees is None else n_trees

    def make():
        rng = np.random.default_rng([0x5CA7, arity])
        f = WideForest()
        top = 2 * arity + 1
        sizes = np.arange(n_trees, dtype=np.int64) % top + 1
        rng.shuffle(sizes)
        sizes[at_trip_borders(n_trees)] = top  # at least two levels on both sides of a trip border
        border = set(trip_borders(n_trees))
        ones = np.nonzero(sizes == 1)[0]
        # a handful of one-leaf trees with limbs >= p: the first, the last, and the nearest to every trip border on both sides
        picks = {int(ones[0]), int(ones[-1])}
        for c in range(TREE_CHUNK, n_trees, TREE_CHUNK):
            j = int(np.searchsorted(ones, c))
            picks |= {int(ones[j - 1]), int(ones[min(j, ones.size - 1)])}
        f.unreduced = sorted(picks - border)
        f.arity, f.sizes, f.off, f.max_leaves = arity, sizes, TS.offsets(sizes, dtype=np.int64), top
        f.flat = leaves(f.off[-1], 0xF0 + arity)
        for i, t in enumerate(f.unreduced):
            f.flat[f.off[t]] = E._PAT_RAW[E._BIG[i % len(E._BIG)]]
        f.oracle_ids = oracle_share(n_trees, f.unreduced, rng)
        return f
    return _cached(("wide", arity, n_trees), make)


def oracle_share(n_trees, extra, rng, n_random=200):
    """the trees the oracle's single-tree build covers: the border trees, trees 0 and n_trees - 1, `extra`, and n_random random ones"""
    ids = set(trip_borders(n_trees)) | {0, n_trees - 1} | {int(t) for t in extra}
    ids |= {int(t) for t in rng.choice(n_trees, min(n_random, n_trees), replace=False)}
    return sorted(ids)


def expected_forest(sizes, off, flat, arity, digest):
    """(roots (T, 4), levels (sum levels_len, 4), lo (T + 1,)) of the forest: the trees grouped by size, their children gathered with
    numpy and zero-padded, digested level by level with digest((m, arity, 4)) -> (m, 4).  A one-leaf tree's root is its leaf mod p, an
    empty tree's is zero."""
    sizes, off = np.asarray(sizes, dtype=np.int64), np.asarray(off, dtype=np.int64)
    lo = TS.block_starts(sizes, arity)
    roots = np.zeros((sizes.size, 4), dtype=np.uint64)
    levels = np.zeros((int(lo[-1]), 4), dtype=np.uint64)
    for n in np.unique(sizes):
        n = int(n)
        ids = np.nonzero(sizes == n)[0]
        if n == 0:
            continue
        cur = flat[off[ids][:, None] + np.arange(n)]  # (m, n, 4)
        if n == 1:
            roots[ids] = E.reduce_mod_p(cur[:, 0])
            continue
        block = []
        while cur.shape[1] > 1:
            up = (cur.shape[1] + arity - 1) // arity
            ch = np.zeros((ids.size, up * arity, 4), dtype=np.uint64)
            ch[:, :cur.shape[1]] = cur
            cur = np.asarray(digest(ch.reshape(ids.size * up, arity, 4))).reshape(ids.size, up, 4)
            block.append(cur)
        block = np.concatenate(block, axis=1)
        levels[lo[ids][:, None] + np.arange(block.shape[1])] = block
        roots[ids] = cur[:, 0]
    return roots, levels, lo


def oracle_digest(arity):
    import oracle
    tag = E._mtag(arity)
    return lambda ch: oracle.hash_batch(tag, np.ascontiguousarray(ch), arity, 1, threads=E.ORACLE_THREADS).reshape(-1, 4)


def oracle_trees(arity, sizes, off, flat, ids):
    """{t: (root, levels)} of the oracle's single-tree build (a one-leaf tree: its leaf mod p, no storage)"""
    tag, tree = E._mtag(arity), E._otree(arity)

    def one(t):
        lv = flat[int(off[t]):int(off[t]) + int(sizes[t])]
        if lv.shape[0] == 1:
            return E.reduce_mod_p(lv[:1])[0], np.zeros((0, 4), dtype=np.uint64)
        root, levels, _ = tree(tag, np.ascontiguousarray(lv), want_levels=True)
        return root, levels
    return dict(zip(ids, E._pmap(one, ids)))


def expected_siblings(sizes, off, flat, lo, levels, tid, lid, arity, stride):
    """(siblings (k, stride, arity - 1, 4), positions (k, stride), depths (k,)) of the openings of (tid, lid) by numpy indexing into
    the leaves and the tree-major levels: the other child slots of the node's parent, ascending, zero at or past the level's width
    and at or past the tree's depth"""
    tid, lid = np.asarray(tid, dtype=np.int64), np.asarray(lid, dtype=np.int64)
    k = tid.size
    sib = np.zeros((k, stride, arity - 1, 4), dtype=np.uint64)
    pos = np.zeros((k, stride), dtype=np.uint8)
    src = np.concatenate([flat, levels])
    start = np.asarray(off, dtype=np.int64)[tid]  # where the node's level starts in src
    node, w = lid.copy(), np.asarray(sizes, dtype=np.int64)[tid]
    depths = np.zeros(k, dtype=np.int64)
    for l in range(stride):
        alive = w > 1
        depths += alive
        p = node % arity
        pos[:, l] = np.where(alive, p, 0)
        for s in range(arity - 1):
            c = node - p + s + (s >= p)
            ok = alive & (c < w)
            sib[ok, l, s] = src[(start + c)[ok]]
        start = np.where(l == 0, flat.shape[0] + np.asarray(lo, dtype=np.int64)[tid], start + w)
        node, w = node // arity, np.where(alive, (w + arity - 1) // arity, w)
    return sib, pos, depths


# ---------------------------------------------------------------------------------------------- append and resize
KEEP_ALL = (1 << 64) - 1


def resize_counts(sizes_old, keep, m, arity):
    """what forest_resize_model (keep None: forest_append_model) gives for a forest of good trees and appends none of which is
    refused: (n_new, n_hashed, n_bad).  sizes_old (T_old,), keep (T_new,) kept counts or None, m (T_new,) appended counts."""
    m = np.asarray(m, dtype=np.int64)
    T = m.size
    n_old = np.zeros(T, dtype=np.int64)
    both = min(T, len(sizes_old))
    n_old[:both] = np.asarray(sizes_old, dtype=np.int64)[:both]
    k = n_old if keep is None else np.minimum(np.asarray(keep, dtype=np.uint64), n_old.astype(np.uint64)).astype(np.int64)
    n_new = k + m
    unchanged = (m == 0) & (k == n_old)
    hashed = 0
    for l, w in enumerate(TS.level_widths(n_new, arity), 1):
        clean = np.where(unchanged, w, np.minimum(k // arity ** l, w))
        hashed += int((w - clean).sum())
    return n_new, hashed, int((n_new == 0).sum())


def resize_leaves(off_old, flat, keep_counts, add_off, add):
    """the new forest's leaves: tree t's first keep_counts[t] old leaves, then add[add_off[t]:add_off[t + 1]]"""
    k, m = np.asarray(keep_counts, dtype=np.int64), np.diff(np.asarray(add_off, dtype=np.int64))
    n_new = k + m
    new_off = TS.offsets(n_new, dtype=np.int64)
    out = np.empty((int(new_off[-1]), 4), dtype=np.uint64)
    T, T_old = k.size, len(off_old) - 1
    old_start = np.zeros(T, dtype=np.int64)
    old_start[:min(T, T_old)] = np.asarray(off_old, dtype=np.int64)[:min(T, T_old)]
    tree = np.repeat(np.arange(T), n_new)
    j = np.arange(int(new_off[-1])) - new_off[tree]
    old = j < k[tree]
    out[old] = flat[(old_start[tree] + j)[old]]
    out[~old] = add[(np.asarray(add_off, dtype=np.int64)[tree] + j - k[tree])[~old]]
    return out, new_off


def wide_append(arity, n_trees=None):
    """one append onto the wide forest: 0 .. 3 leaves onto a random quarter of the trees, the border trees among them, and one
    tile + 3 new trees -> dict(m, add_off, add, T_new, max_new)"""
    def make():
        f = wide_forest(arity, n_trees)
        rng = np.random.default_rng([0xA99, arity])
        T, T_new = f.sizes.size, f.sizes.size + TREE_TILE + 3
        m = np.zeros(T_new, dtype=np.int64)
        m[:T] = np.where(rng.random(T) < 0.25, rng.integers(0, 4, T), 0)
        m[trip_borders(T)] = rng.integers(1, 4, len(trip_borders(T)))
        m[T:] = rng.integers(1, f.max_leaves + 1, T_new - T)
        add_off = TS.offsets(m, dtype=np.int64)
        return dict(m=m, add_off=add_off, add=leaves(add_off[-1], 0xAD + arity), T_new=T_new, max_new=f.max_leaves + 3, keep=None)
    return _cached(("append", arity, n_trees), make)


def wide_resize(arity, sizes):
    """one resize of a forest of `sizes` (the append's result): 1 .. 2 leaves off a random quarter, some trees cut to one leaf, the last
    tile + 7 trees dropped, leaves appended in the same call (to cut and uncut trees, the border trees of the new numbering among them)"""
    def make():
        rng = np.random.default_rng([0x2E5, arity])
        sizes_ = np.asarray(sizes, dtype=np.int64)
        T_new = sizes_.size - (TREE_TILE + 7)
        n = sizes_[:T_new]
        keep = np.full(T_new, KEEP_ALL, dtype=np.uint64)
        cut = rng.random(T_new) < 0.25
        keep[cut] = np.maximum(n[cut] - rng.integers(1, 3, int(cut.sum())), 1).astype(np.uint64)
        to_one = rng.choice(T_new, min(3000, T_new // 4), replace=False)
        keep[to_one] = 1
        b = trip_borders(T_new)
        keep[b[0::2]] = np.maximum(n[b[0::2]] - 1, 1).astype(np.uint64)  # (the tree before each border is cut, the one after it grows)
        m = np.where(rng.random(T_new) < 0.2, rng.integers(1, 3, T_new), 0)
        m[b] = 2
        to_zero = np.setdiff1d(rng.choice(T_new, 6, replace=False), b)  # cut to nothing, nothing appended: empty trees, counted bad
        to_zero = np.union1d(to_zero, [T_new - 2])
        keep[to_zero], m[to_zero] = 0, 0
        add_off = TS.offsets(m, dtype=np.int64)
        return dict(m=m, add_off=add_off, add=leaves(add_off[-1], 0x2E + arity), T_new=T_new, max_new=int(sizes_.max()) + 2, keep=keep,
                    to_one=to_one, to_zero=to_zero)
    return _cached(("resize", arity, len(sizes)), make)


# ---------------------------------------------------------------------------------------------- single-tree multiproofs
def single_n(arity):
    return 4 ** 9 + 1 if arity == 4 else 2 ** 18 + 1


def dense(n, seed=50):
    """every leaf except a random one of every 50 (the last leaf stays): no parent loses all of its children"""
    rng = np.random.default_rng(seed)
    keep = np.ones(n, dtype=bool)
    starts = np.arange(0, n - 1, 50)
    span = np.minimum(50, n - 1 - starts)
    keep[starts + (rng.integers(0, 50, starts.size) % span)] = False
    return np.nonzero(keep)[0].astype(np.int64)


def sparse(n, k=140000, seed=51):
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False)).astype(np.int64)


def single_positions(arity, case):
    n = single_n(arity)
    return _cached(("pos", arity, case), lambda: dense(n) if case == "dense" else sparse(n))


# ---------------------------------------------------------------------------------------------- forest multiproofs
def forest_multiproof_fast(sizes, tid, lid, arity, off=None, flat=None, lo=None, levels=None):
    """forest_multiproof_counts and forest_multiproof_extract of multiproofmodel, vectorised over all trees at once -> dict(po (T + 1,)
    uint64, hashed, counts [|S_0|, |S_1|, ..] (the lists the device walks), and with the forest given: out (k, 4), proof (len, 4))"""
    sizes = np.asarray(sizes, dtype=np.int64)
    t, node = np.asarray(tid, dtype=np.int64).reshape(-1), np.asarray(lid, dtype=np.int64).reshape(-1)
    assert t.size and bool(np.all(np.diff(t * (1 << 40) + node) > 0)) and int(node.min()) >= 0 and bool(np.all(node < sizes[t]))
    extract = flat is not None
    if extract:
        off, lo = np.asarray(off, dtype=np.int64), np.asarray(lo, dtype=np.int64)
        start = off[t]  # where the element's level starts in concatenate([flat, levels])
    else:
        start = np.zeros_like(t)
    w = sizes[t]
    counts, hashed, level = [int(t.size)], 0, 0
    p_tree, p_src = [], []
    while True:
        alive = w > 1
        t, node, w, start = t[alive], node[alive], w[alive], start[alive]
        if not t.size:
            break
        key = t * (1 << 40) + node
        pk, first = np.unique(t * (1 << 40) + node // arity, return_index=True)
        pt, pn, pw, pstart = pk >> 40, pk & ((1 << 40) - 1), w[first], start[first]
        slots = pn[:, None] * arity + np.arange(arity)
        missing = (slots < pw[:, None]) & ~np.isin(pt[:, None] * (1 << 40) + slots, key)
        rows = np.nonzero(missing)[0]  # parent by parent, slot by slot: the visiting order
        p_tree.append(pt[rows])
        p_src.append(pstart[rows] + slots[missing])
        if extract:
            start = np.where(level == 0, flat.shape[0] + lo[pt], pstart + pw)
        else:
            start = pstart
        t, node, w = pt, pn, (pw + arity - 1) // arity
        hashed += int(pt.size)
        counts.append(int(pt.size))
        level += 1
    p_tree = np.concatenate(p_tree) if p_tree else np.zeros(0, dtype=np.int64)
    lens = np.zeros(sizes.size + 1, dtype=np.uint64)
    lens[1:] = np.bincount(p_tree, minlength=sizes.size)
    res = dict(po=np.cumsum(lens, dtype=np.uint64), hashed=hashed, counts=counts)
    if extract:
        order = np.argsort(p_tree, kind="stable")  # tree-major; inside a tree level by level, inside a level the visiting order
        src = np.concatenate([flat, levels])
        res["proof"] = src[np.concatenate(p_src)[order]]
        res["out"] = flat[off[np.asarray(tid, dtype=np.int64)] + np.asarray(lid, dtype=np.int64)]
    return res


class FmCase:
    """arity, sizes, off, max_leaves, tid, lid, victim (a tree behind the second chunk border whose leaf value is changed), big
    (the tree whose part goes through the single-tree verify, or None)"""


def _case(arity, sizes, tid, lid, victim, big=None, seed=0):
    c = FmCase()
    c.arity, c.sizes, c.off, c.max_leaves = arity, np.asarray(sizes, dtype=np.int64), TS.offsets(sizes, dtype=np.int64), int(np.max(sizes))
    c.tid, c.lid, c.victim, c.big, c.seed = np.asarray(tid, dtype=np.int64), np.asarray(lid, dtype=np.int64), int(victim), big, seed
    return c


def _small_pairs(sizes, ids, rng):
    """1 .. 2 pairs in each listed tree: a random leaf, and the last leaf on a coin"""
    ids = np.asarray(ids, dtype=np.int64)
    n = np.asarray(sizes, dtype=np.int64)[ids]
    a = (rng.random(ids.size) * n).astype(np.int64)
    second = (rng.random(ids.size) < 0.5) & (a < n - 1)
    tid = np.concatenate([ids, ids[second]])
    lid = np.concatenate([a, n[second] - 1])
    order = np.lexsort((lid, tid))
    return tid[order], lid[order]


def fm_wide(arity):
    """the wide forest with pairs in about every fourth tree (the border trees among them)"""
    def make():
        f = wide_forest(arity)
        rng = np.random.default_rng([0xF3, arity])
        pick = rng.random(f.sizes.size) < 0.26
        pick[trip_borders(f.sizes.size)] = True
        tid, lid = _small_pairs(f.sizes, np.nonzero(pick)[0], rng)
        victim = int(tid[2 * LIST_CHUNK + 1000])
        return _case(arity, f.sizes, tid, lid, victim)
    return _cached(("fm_wide", arity), make)


def fm_long_run(arity):
    """three small trees, one tree of single_n leaves with the dense positions, a few small trees"""
    def make():
        rng = np.random.default_rng([0xF4, arity])
        sizes = [5, 1, 9, single_n(arity), 7, 1, 2 * arity + 1, 3]
        parts = [(0, [0, 3]), (1, [0]), (2, [2, 8]), (3, dense(single_n(arity))), (4, [1, 6]), (5, [0]), (6, [0, 1, 2 * arity]), (7, [2])]
        tid = np.concatenate([np.full(len(p), t) for t, p in parts])
        lid = np.concatenate([np.asarray(p, dtype=np.int64) for _, p in parts])
        return _case(arity, sizes, tid, lid, 6, big=3, seed=int(rng.integers(1 << 30)))
    return _cached(("fm_long", arity), make)


def fm_aligned(arity, shift):
    """a tree whose first pair is element LIST_CHUNK - 1 + shift of the pair list (shift 0, 1, 2), a long tree behind it that runs over
    the second chunk border, and two small trees behind that"""
    def make():
        rng = np.random.default_rng([0xF5, arity, shift])
        n0 = LIST_CHUNK + LIST_CHUNK // 16
        sizes = [n0, 3000, n0, 2 * arity + 1, 1]
        first = np.sort(rng.choice(n0, LIST_CHUNK - 1 + shift, replace=False))
        parts = [(0, first), (1, np.sort(rng.choice(3000, 2000, replace=False))), (2, np.sort(rng.choice(n0, LIST_CHUNK + 500, replace=False))),
                 (3, [1, 2 * arity]), (4, [0])]
        tid = np.concatenate([np.full(len(p), t) for t, p in parts])
        lid = np.concatenate([np.asarray(p, dtype=np.int64) for _, p in parts])
        return _case(arity, sizes, tid, lid, 3)  # (one set of leaves for the three shifts)
    return _cached(("fm_aligned", arity, shift), make)


FM_CASES = {"wide": fm_wide, "long_run": fm_long_run, "aligned0": lambda a: fm_aligned(a, 0), "aligned1": lambda a: fm_aligned(a, 1),
            "aligned2": lambda a: fm_aligned(a, 2)}


def fm_leaves(case_name, arity):
    """the case's leaves: the wide forest's own, or random scalars"""
    c = FM_CASES[case_name](arity)
    return wide_forest(arity).flat if case_name == "wide" else leaves(c.off[-1], 0x77 + arity + c.seed % 1000)


def first_pair_index(c):
    """{tree: the index of its first pair in the list}"""
    trees, first = np.unique(c.tid, return_index=True)
    return dict(zip(trees.tolist(), first.tolist()))


# ---------------------------------------------------------------------------------------------- the ragged hash
RAGGED_MAX_LEN = 4 * 2 * C["RAGGED_EXACT_BLOCKS"] + 1
_E4 = 4 * C["RAGGED_EXACT_BLOCKS"]
# the last exact bucket (4,091 and 4,092 at 1,024 blocks a bucket), the first octave bucket, a sub-bucket border, max_len itself
RAGGED_LONG = [_E4 - 5, _E4 - 4, _E4 - 3, _E4, _E4 + 1, 6000, 2 * _E4 - 4, 2 * _E4 - 3, 2 * _E4, 2 * _E4 + 1, _E4 - 3, 2 * _E4 + 1]


def ragged_batch(n, seed=0):
    """(flat, offsets uint64 (n + 1,), lens): n messages, mostly 1 .. 42 scalars, the twelve long ones spread among them"""
    rng = np.random.default_rng([0x7A6, n, seed])
    lens = rng.integers(1, 43, n)
    at = np.sort(rng.choice(n, len(RAGGED_LONG), replace=False))
    lens[at] = RAGGED_LONG
    off = TS.offsets(lens)
    return leaves(int(off[-1]), 0x7A + n), off, lens


def ragged_oracle(flat, off, out_len):
    """the oracle's digests: one run per distinct length with that length's tag (domain Other)"""
    import oracle
    lens = np.diff(off.astype(np.int64))
    out = np.zeros((lens.size, out_len, 4), dtype=np.uint64)

    def one(L):
        sel = np.nonzero(lens == L)[0]
        x = flat[off[sel].astype(np.int64)[:, None] + np.arange(L)]
        return sel, oracle.hash_batch(oracle.tag(3, [L], out_len), np.ascontiguousarray(x), L, out_len, threads=1)
    for sel, digests in E._pmap(one, [int(L) for L in np.unique(lens)[::-1]]):  # (the long messages first: one thread each)
        out[sel] = digests
    return out


def blocks_of(length):
    return -(-int(length) // 4)


# ---------------------------------------------------------------------------------------------- the runners (need torch and a GPU)
def _call(ctx, arity, stem):
    return getattr(ctx, "merkle%d_forest_ragged_%s" % (arity, stem))


def run_build(ctx, arity, flat, off, max_leaves, want_levels=True, d=None):
    """one build into sentinel buffers -> (d_leaves, d_off, d_roots, d_levels or None, n_bad)"""
    import torch
    T = len(off) - 1
    d = E._dev(flat) if d is None else d
    d_off = E._dev(np.asarray(off, dtype=np.uint64))
    roots = torch.full((T, 4), SENTINEL, dtype=torch.int64, device=d.device)
    lv = torch.full((max(TS.levels_bound(flat.shape[0], T, max_leaves, arity), 1), 4), SENTINEL, dtype=torch.int64, device=d.device) if want_levels else None
    bad = torch.zeros(1, dtype=torch.int32, device=d.device)
    ctx.merkle_forest_ragged_device(E._mtag(arity), d, d_off, T, max_leaves, roots, lv, bad, arity=arity)
    torch.cuda.synchronize()
    return d, d_off, roots, lv, int(bad)


def run_resize(ctx, arity, old, step, n_leaves_old):
    """the append (step['keep'] None) or the resize of the forest old = (d_leaves, d_off, T, max_leaves, d_levels) into sentinel
    buffers -> (d_leaves_new, d_off_new, d_levels_new, d_roots, n_bad, n_hashed)"""
    import torch
    d, d_off, T, maxl, d_lv = old
    T2, max_new, n_add = step["T_new"], step["max_new"], int(step["add_off"][-1])
    total = n_leaves_old + n_add
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device=d.device)  # noqa: E731
    o_leaves, o_off, o_lv, o_roots = full(total, 4), full(T2 + 1), full(max(TS.levels_bound(total, T2, max_new, arity), 1), 4), full(T2, 4)
    bad, hashed = torch.zeros(1, dtype=torch.int32, device=d.device), torch.zeros(1, dtype=torch.int64, device=d.device)
    args = (E._mtag(arity), d, d_off, T, maxl, d_lv)
    keep = () if step["keep"] is None else (E._dev(step["keep"]),)
    _call(ctx, arity, "append_device" if step["keep"] is None else "resize_device")(
        *args, *keep, E._dev(step["add"]), E._dev(step["add_off"].astype(np.uint64)), T2, max_new, o_leaves, o_off, o_lv, o_roots, bad, hashed)
    torch.cuda.synchronize()
    return o_leaves, o_off, o_lv, o_roots, int(bad), int(hashed)


def run_forest_multiproof(ctx, c, flat, built=None):
    """extract + verify of the case's pairs on a forest built here (or `built` = run_build's result) -> dict of host arrays"""
    import torch
    a, T, k = c.arity, c.sizes.size, c.tid.size
    d, d_off, roots, lv, bad0 = built if built is not None else run_build(ctx, a, flat, c.off, c.max_leaves)
    n = flat.shape[0]
    bound = _call(ctx, a, "multiproof_bound")(n, T, c.max_leaves, k)
    dev = d.device
    out = torch.full((k, 4), SENTINEL, dtype=torch.int64, device=dev)
    proof = torch.full((bound + 5, 4), SENTINEL, dtype=torch.int64, device=dev)
    po = torch.full((T + 1,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    d_tid, d_lid = E._dev(c.tid.astype(np.uint32)), E._dev(c.lid.astype(np.uint64))
    _call(ctx, a, "multiproof_device")(d, d_off, T, c.max_leaves, lv, d_tid, d_lid, k, out, proof[:bound], po, bad[:1])
    torch.cuda.synchronize()
    length = int(po[-1])
    res = dict(build_bad=bad0, roots=E._host(roots), po=E._host(po), length=length, bound=bound, out=E._host(out), proof=E._host(proof))
    assert 0 <= length <= bound, "proof_offsets[-1] = %d is outside the bound %d" % (length, bound)

    def verify(d_out):
        ok = torch.full((T,), 7, dtype=torch.uint8, device=dev)
        r_out = torch.full((T, 4), SENTINEL, dtype=torch.int64, device=dev)
        hashed = torch.full((1,), -1, dtype=torch.int64, device=dev)
        _call(ctx, a, "multiproof_verify_device")(E._mtag(a), d_off, n, T, c.max_leaves, d_tid, d_lid, d_out, k, proof[:length] if length else None,
                                                  length, po, roots, ok, r_out, hashed, bad[1:])
        torch.cuda.synchronize()
        return E._host(ok), E._host(r_out), int(hashed)
    res["ok"], res["roots_out"], res["hashed"] = verify(out)
    changed = out.clone()
    j = first_pair_index(c)[c.victim]
    changed[j, 0] = changed[j, 0] ^ 1  # one changed leaf value of the victim tree
    res["ok_changed"], _, _ = verify(changed)
    res["bad"] = E._host(bad).tolist()
    res["d"] = (d, d_off, roots, lv, out, proof, po)
    return res


def run_ragged(ctx, n, out_len, truncated):
    import torch
    from poseidon252_amd import hash as H
    flat, off, _ = ragged_batch(n)
    d_tags = E._dev(H.ragged_tags(H.Domain.Other, out_len, RAGGED_MAX_LEN))
    out = torch.full((n, out_len, 4), SENTINEL, dtype=torch.int64, device="cuda:0")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ctx.hash_ragged_device(d_tags, RAGGED_MAX_LEN, E._dev(flat), E._dev(off), out_len, out, n, d_n_bad=bad, truncated=truncated)
    torch.cuda.synchronize()
    assert int(bad) == 0
    return E._host(out)


def _digest_of(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def child(what, arity, out_dir):
    """one runner in this (fresh) process, its outputs saved under out_dir: what = build | fm:<case> | ragged"""
    import poseidon252_amd as P
    ctx = P.Context(0)
    if what == "build":
        f = wide_forest(arity)
        _, _, roots, lv, bad = run_build(ctx, arity, f.flat, f.off, f.max_leaves)
        used = int(TS.levels_len(f.sizes, arity).sum())
        np.savez(os.path.join(out_dir, "build.npz"), roots=E._host(roots), levels_sha256=_digest_of(E._host(lv)[:used]), bad=bad)
    elif what.startswith("fm:"):
        name = what[3:]
        c = FM_CASES[name](arity)
        r = run_forest_multiproof(ctx, c, fm_leaves(name, arity))
        np.savez(os.path.join(out_dir, "fm.npz"), po=r["po"], proof=r["proof"][:r["length"]], ok=r["ok"], ok_changed=r["ok_changed"],
                 roots_out=r["roots_out"], hashed=r["hashed"])
    else:
        outs = {"%d_%d_%d" % (n, ol, tr): run_ragged(ctx, n, ol, bool(tr)) for n in RAGGED_SIZES for ol in (1, 5) for tr in (0, 1)}
        np.savez(os.path.join(out_dir, "ragged.npz"), **outs)
    print("done")


RAGGED_SIZES = (9000, 100)

if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
