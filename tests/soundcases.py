"""The shapes of the soundness sweep, once: the good proofs (out of the oracle's trees), every change to them (testsupport/soundness.py)
and the model's verdict for each, computed on the host and cached — tests/test_soundness_cpu.py checks the catalogue and the model
against each other, tests/test_soundness_gpu.py puts the same cases to the device.  A plain helper module, as shapecases and edgecases
are.  Nothing here touches a GPU."""
import functools

import numpy as np

import oracle
from edgecases import ORACLE_THREADS, _mtag
from helpers.forest import _mix
from testsupport import multiproofmodel as MM
from testsupport import soundness as S
from testsupport import treeshape as TS

SHARED_SHAPES = {4: (1, 2, 4, 5, 16, 17, 21, 64, 65), 2: (1, 2, 3, 7, 8, 9, 33)}
COPIES_SHAPES = {4: (21, 65), 2: (9, 33)}
TILE_SHAPES = {4: 4 ** 5 + 5, 2: 2 ** 10 + 1}
TILE = 256  # elements per scan tile of k_mp_apply
FIXED_TREES = {4: ((3, 4 ** 3), (3, 21), (4, 4 ** 4), (4, 65)), 2: ((3, 2 ** 3), (4, 2 ** 4), (4, 9), (6, 33))}  # (depth, leaves)
ANCHOR_SIZES = {4: [1, 2, 4, 5, 15, 16, 17, 37, 70], 2: [1, 2, 2, 3, 3, 4, 5, 37]}  # test_forest_anchor_gpu's small forest
MANY_TREES, MANY_PAIRS = 3000, 12


_MEMO = {4: {}, 2: {}}


def digest(arity):
    """the oracle's node digest; small batches remember what they hashed (the cases of one tree share nearly all their nodes)"""
    tag, memo = _mtag(arity), _MEMO[arity]

    def run(kids, remember=False):
        kids = np.ascontiguousarray(kids, dtype=np.uint64).reshape(-1, arity, 4)
        if len(kids) > 2048 and not remember:
            return oracle.hash_batch(tag, kids, arity, 1, threads=ORACLE_THREADS).reshape(-1, 4)
        keys = [row.tobytes() for row in kids]
        miss = [i for i, key in enumerate(keys) if key not in memo]
        if miss:
            for i, out in zip(miss, oracle.hash_batch(tag, kids[miss], arity, 1, threads=ORACLE_THREADS if len(miss) > 2048 else 1).reshape(-1, 4)):
                memo[keys[i]] = out
        return np.array([memo[key] for key in keys], dtype=np.uint64).reshape(-1, 4)
    return run


def _leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60): V + p stays below 2^256"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(n, 4), dtype=np.uint64)


def _build(arity, leaves):
    """(root, levels) of the oracle's tree; one leaf is its own root"""
    root, levels = (oracle.merkle4_tree if arity == 4 else oracle.merkle2_tree)(_mtag(arity), leaves, want_levels=True)[:2]
    return np.asarray(root, dtype=np.uint64), levels


def _build_forest(arity, flat, off):
    """[(root, levels)] of the trees flat[off[t]:off[t + 1]] of two leaves or more, a level of ALL trees per call of the digest, which
    remembers the nodes (the model then hashes only what a case changed)"""
    cur, levels = [flat[off[t]:off[t + 1]] for t in range(len(off) - 1)], [[] for _ in range(len(off) - 1)]
    while max(len(c) for c in cur) > 1:
        todo = [t for t, c in enumerate(cur) if len(c) > 1]
        kids = []
        for t in todo:
            up = (len(cur[t]) + arity - 1) // arity
            padded = np.zeros((up * arity, 4), dtype=np.uint64)
            padded[:len(cur[t])] = cur[t]
            kids.append(padded.reshape(up, arity, 4))
        out = digest(arity)(np.concatenate(kids), remember=True)
        at = 0
        for t, k in zip(todo, kids):
            cur[t] = out[at:at + len(k)]
            levels[t].append(cur[t])
            at += len(k)
    return [(c[0].copy(), np.concatenate(lv)) for c, lv in zip(cur, levels)]


@functools.lru_cache(maxsize=None)
def tree(arity, n):
    leaves = _leaves(n, 7000 * arity + n)
    return (leaves,) + _build(arity, leaves)


def _good(arity, n, pos):
    leaves, root, levels = tree(arity, n)
    return S.shared_good(leaves, levels, pos, root, arity, spare=_leaves(1, n)[0])


# ---------------------------------------------------------------------------------------------- shared proof, one tree
@functools.lru_cache(maxsize=None)
def shared_single(arity, n):
    """[(set name, good inputs, cases, the model's verdicts)] for every position set of a tree of n leaves"""
    rng, out = np.random.default_rng(100 * n + arity), []
    for name, pos in S.index_sets(n, arity).items():
        x = _good(arity, n, pos)
        cases = [("good", x, S.ACCEPT)] + S.shared_cases(x, arity, rng)
        out.append((name, x, cases, [S.shared_verdict(c, arity, digest(arity)) for _, c, _ in cases]))
    return out


@functools.lru_cache(maxsize=None)
def shared_tiles(arity):
    """(good inputs, the proof scalars next to a tile border, cases, verdicts): every other leaf of a tree whose levels 0 (and up) hold
    more than one scan tile; the flips, + p and swap of the proof scalars of the parents on either side of each border and of the last"""
    n = TILE_SHAPES[arity]
    x = _good(arity, n, np.arange(0, n, 2))
    nodes, sets, _ = MM.multiproof_model(n, x["pos"], arity)
    at, start = {x["plen"] - 1}, 0
    for l, level in enumerate(nodes):
        for b in range(TILE, sets[l].size, TILE):
            parents = {int(sets[l][b - 1]) // arity, int(sets[l][b]) // arity}
            at |= {start + j for j, c in enumerate(level.tolist()) if c // arity in parents}
        start += level.size
    at = sorted(at)
    cases = [("good", x, S.ACCEPT)] + S.shared_cases(x, arity, np.random.default_rng(arity), proof_at=at)
    return x, at, cases, [S.shared_verdict(c, arity, digest(arity)) for _, c, _ in cases]


# ---------------------------------------------------------------------------------------------- shared proof, a forest
@functools.lru_cache(maxsize=None)
def shared_copies(arity, n):
    """(forest inputs, the tree of case i, cases, the model's verdict): copies of one tree, one case each, every position set in turn"""
    rng, cases = np.random.default_rng(200 * n + arity), []
    for pos in S.index_sets(n, arity).values():
        x = _good(arity, n, pos)
        cases += [("good", x, S.ACCEPT)] + S.shared_cases(x, arity, rng, in_range_only=True)
    trees, where = S.copies_forest(cases, _good(arity, n, [0]))
    F = S.forest_of(trees)
    return F, where, cases, S.forest_verdict(F, arity, digest(arity))


@functools.lru_cache(maxsize=None)
def many_good(arity=4):
    """the "many" forest of test_forest_multiproof_gpu (3,000 trees of 16 .. 40 leaves, 12 pairs each): the good inputs of every tree"""
    sizes = np.random.default_rng(77).integers(16, 41, size=MANY_TREES)
    off = TS.offsets(sizes, dtype=np.int64)
    flat = _leaves(int(off[-1]), 31 * arity + MANY_TREES)
    rng, out = np.random.default_rng(9), []
    built = _build_forest(arity, flat, off)
    for t, n in enumerate(sizes):
        leaves = flat[off[t]:off[t + 1]]
        root, levels = built[t]
        out.append(S.shared_good(leaves, levels, np.sort(rng.choice(int(n), MANY_PAIRS, replace=False)), root, arity, spare=flat[0]))
    return out


@functools.lru_cache(maxsize=None)
def shared_many(every, arity=4):
    """(forest inputs, the class put into each tree or None, the model's verdict): one random case — none that moves an offset — in every
    `every`-th tree of the many forest"""
    rng, trees, classes = np.random.default_rng(300 + every), [], []
    for t, x in enumerate(many_good(arity)):
        if t % every:
            trees.append(x), classes.append(None)
            continue
        cls, c, _ = S.shared_one(x, arity, rng, skip=S.LIES)
        trees.append(c), classes.append(cls)
    F = S.forest_of(trees)
    return F, classes, S.forest_verdict(F, arity, digest(arity))


# ---------------------------------------------------------------------------------------------- openings
def _swept(O, arity, ragged, seed):
    rng = np.random.default_rng(seed)
    B, cls, exp, rows = S.opening_cases(O, arity, rng, ragged)
    changed = [(name, roots, S.openings_verdict(dict(O, roots=roots), arity, digest(arity))) for name, roots in S.root_cases(O, rng)]
    return dict(good=O, batch=B, cls=cls, exp=exp, rows=rows, ok=S.openings_verdict(B, arity, digest(arity)), roots=changed)


@functools.lru_cache(maxsize=None)
def fixed_openings(arity, depth, n):
    """every case of every leaf's opening of a tree of n leaves (depth `depth`) in one batch, for p252_merkle{4,2}_verify_batch_device"""
    leaves, root, levels = tree(arity, n)
    assert TS.depth(n, arity) == depth
    return _swept(S.openings_good([S.open_tree(leaves, levels, arity, depth) + (root,)], depth), arity, False, 400 * arity + n)


@functools.lru_cache(maxsize=None)
def ragged_openings(arity):
    """the same for every leaf of the trees of helpers.forest._mix(arity) at one stride, with the depth byte, the tree id and the rows past
    the depth, for p252_merkle{4,2}_forest_ragged_verify_device"""
    sizes = _mix(arity)
    D, parts = int(TS.depth(max(sizes), arity)), []
    for t, n in enumerate(sizes):
        leaves = _leaves(n, 500 * arity + t)
        root, levels = _build(arity, leaves)
        parts.append(S.open_tree(leaves, levels, arity, D) + (root,))
    return _swept(S.openings_good(parts, D), arity, True, 600 + arity)


def anchor_forest(arity):
    """(sizes, the trees' leaves, the anchors' trees and counts, the openings' anchors and leaves): every tree of two leaves or more as it
    was at two earlier counts — one leaf less, and half of them — and every leaf under each anchor"""
    sizes = ANCHOR_SIZES[arity]
    trees = [_leaves(n, 700 * arity + t) for t, n in enumerate(sizes)]
    a_tree = [t for t, n in enumerate(sizes) if n >= 2 for _ in range(2)]
    a_count = [c for n in sizes if n >= 2 for c in (n - 1, (n + 1) // 2)]
    o_anchor = np.repeat(np.arange(len(a_tree)), a_count)
    o_leaf = np.concatenate([np.arange(c) for c in a_count])
    return sizes, trees, np.array(a_tree), np.array(a_count), o_anchor, o_leaf


@functools.lru_cache(maxsize=None)
def anchored_openings(arity):
    """the ragged sweep on anchored openings: tree t at its first c leaves is the oracle's tree of those leaves"""
    sizes, trees, a_tree, a_count, _, _ = anchor_forest(arity)
    D, parts = int(TS.depth(max(sizes), arity)), []
    for t, c in zip(a_tree, a_count):
        root, levels = _build(arity, trees[t][:c])
        parts.append(S.open_tree(trees[t][:c], levels, arity, D) + (S.reduce_mod_p(root),))
    return _swept(S.openings_good(parts, D), arity, True, 800 + arity)
