"""Leaf updates of a ragged forest applied in order, each with its witness (p252_merkle{4,2}_forest_ragged_update_sequential_device_into;
csrc/forest_sequential.hip) on the GPU: every output against the numpy model of one-by-one application (testsupport/forestsequential.py)
byte for byte, the forest afterwards against a fresh build, the witnesses through path_ragged_device; the three extremes of the merge;
a batch past the lane-group rule; every kind of bad update and of bad order; distinct pairs against update_device; leaves at and above
the modulus; two streams of one context; the convenience."""
import numpy as np
import pytest

import edgecases as E
from helpers.forest import SENTINEL, _np, _tag, _torch, _update
from testsupport import forestsequential as FS
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

SENT64 = np.uint64(SENTINEL & (2 ** 64 - 1))
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257]
_HOST = {}


def _leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60)"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(n, 4), dtype=np.uint64)


def _digest(oracle_mod, arity):
    """the node hash of (m, arity, 4) children, which may hold words at and above the modulus: the oracle gets them reduced"""
    def digest(kids):
        kids = np.ascontiguousarray(kids, dtype=np.uint64)
        return oracle_mod.hash_batch(_tag(arity), E.reduce_mod_p(kids.reshape(-1, 4)).reshape(kids.shape), arity, 1)
    return digest


def _host_trees(oracle_mod, arity, sizes, leaves, name):
    """the model's trees of a forest, built once per (arity, name) with the oracle's digests and copied for every test"""
    if (arity, name) not in _HOST:
        _HOST[(arity, name)] = FS.build_forest(leaves, sizes, arity, _digest(oracle_mod, arity))
    return [None if t is None else [row.copy() for row in t] for t in _HOST[(arity, name)]]


class Forest:
    """a forest built on the device with its levels, in sentinel-filled buffers with a tail"""

    def __init__(self, ctx, arity, sizes, leaves, max_leaves=None):
        import torch
        self.ctx, self.arity, self.sizes, self.T = ctx, arity, list(sizes), len(sizes)
        self.top = int(max(sizes)) if max_leaves is None else max_leaves
        self.off = TS.offsets(sizes, dtype=np.int64)
        self.n = int(self.off[-1])
        self.d, self.d_off = _torch(leaves), _torch(self.off.astype(np.uint64))
        self.bound = max(TS.levels_bound(self.n, self.T, self.top, arity), 1)
        self.d_lv = torch.full((self.bound + 5, 4), SENTINEL, dtype=torch.int64, device=self.d.device)
        self.d_roots = torch.full((self.T, 4), SENTINEL, dtype=torch.int64, device=self.d.device)
        ctx.merkle_forest_ragged_device(_tag(arity), self.d, self.d_off, self.T, self.top, self.d_roots, d_levels=self.d_lv, arity=arity)
        self.D = int(TS.depth(self.top, arity))

    def state(self):
        import torch
        torch.cuda.synchronize()
        return _np(self.d).copy(), _np(self.d_lv).copy(), _np(self.d_roots).copy()


def _launch(f, tid, lid, new, order=None, optional=True):
    """enqueues one call on numpy inputs on the current stream -> its device buffers, each with one sentinel row behind"""
    import torch
    k, D, per = len(tid), f.D, f.arity - 1
    dev = f.d.device
    order = FS.stable_order(tid, lid) if order is None else np.asarray(order, dtype=np.uint32)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device=dev)  # noqa: E731
    b = dict(old=full(k + 1, 4), before=full(k + 1, 4), after=full(k + 1, 4), sib=full(k * D * per + 1, 4),
             pos=torch.full((k * D + 1,), 7, dtype=torch.uint8, device=dev), dep=torch.full((k + 1,), 7, dtype=torch.uint8, device=dev),
             bad=torch.zeros(1, dtype=torch.int32, device=dev), hashed=torch.zeros(1, dtype=torch.int64, device=dev))
    call = f.ctx.merkle4_forest_ragged_update_sequential_device if f.arity == 4 else f.ctx.merkle2_forest_ragged_update_sequential_device
    call(_tag(f.arity), f.d, f.d_off, f.T, f.top, f.d_lv if D else None, _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64)),
         _torch(np.ascontiguousarray(new, dtype=np.uint64)), _torch(order), k, b["sib"] if D else None, b["pos"] if D else None, b["dep"][:k], b["after"],
         d_old_leaves=b["old"] if optional else None, d_roots_before=b["before"] if optional else None, d_roots=f.d_roots if optional else None,
         d_n_bad=b["bad"], d_n_hashed=b["hashed"])
    return b


def _read(f, b):
    """-> dict of numpy outputs (nothing past the k-th row was written), n_bad, n_hashed"""
    import torch
    torch.cuda.synchronize()
    k, D, per = b["dep"].shape[0] - 1, f.D, f.arity - 1
    out = {name: _np(b[name]) for name in ("old", "sib", "pos", "dep", "before", "after")}
    for name, a in out.items():
        assert (a[-1] == (7 if a.dtype == np.uint8 else SENT64)).all(), name
    out = {n: a[:-1] for n, a in out.items()}
    out["sib"], out["pos"] = out["sib"].reshape(k, D, per, 4), out["pos"].reshape(k, D)
    out["d"] = dict(old=b["old"][:k], sib=b["sib"][:k * D * per], pos=b["pos"][:k * D], dep=b["dep"][:k])
    return out, int(b["bad"]), int(b["hashed"])


def _call(f, tid, lid, new, order=None, optional=True):
    return _read(f, _launch(f, tid, lid, new, order, optional))


def _same_as_model(out, W):
    for name in ("old", "sib", "pos", "dep", "before", "after"):
        assert np.array_equal(out[name], getattr(W, name)), name


def _forest_is_the_models(f, trees, untouched_roots=None):
    """leaves, the used levels and the roots equal the model's trees: a fresh build of the final leaves; the tail keeps the sentinel"""
    leaves, levels, roots = FS.forest_arrays(trees, E.reduce_mod_p)
    d, lv, r = f.state()
    assert np.array_equal(d, leaves)
    assert np.array_equal(lv[:len(levels)], levels) and (lv[len(levels):] == SENT64).all()
    if untouched_roots is None:
        assert np.array_equal(r, roots)
    else:  # d_roots is rewritten for the trees that received a good update only
        assert np.array_equal(r[~untouched_roots], roots[~untouched_roots]) and np.array_equal(r[untouched_roots], f.roots0[untouched_roots])


def _rehash(f, out, new):
    """path_ragged_device on (old leaf, opening) and on (new leaf, the same opening) -> the two (k, 4) arrays of roots"""
    import torch
    k = out["dep"].shape[0]
    d = out["d"]
    res = []
    for leaves in (d["old"], _torch(np.ascontiguousarray(new, dtype=np.uint64))):
        back = torch.full((k, 4), SENTINEL, dtype=torch.int64, device=f.d.device)
        f.ctx.merkle_path_ragged_device(_tag(f.arity), leaves, d["sib"] if f.D else None, d["pos"] if f.D else None, d["dep"], f.D, back, k, arity=f.arity)
        res.append(back)
    f.ctx.sync()
    return _np(res[0]), _np(res[1])


def _twelve(ctx, oracle_mod, arity):
    leaves = _leaves(sum(SIZES), 91 * arity)
    f = Forest(ctx, arity, SIZES, leaves)
    f.roots0 = f.state()[2]
    return f, _host_trees(oracle_mod, arity, SIZES, leaves, "twelve")


def _run_against_model(f, trees, oracle_mod, tid, lid, new):
    W = FS.sequential_model(trees, tid, lid, new, f.top, f.arity, _digest(oracle_mod, f.arity), E.reduce_mod_p)
    out, bad, hashed = _call(f, tid, lid, new)
    print("arity %d: %d updates, bad %d (model %d), n_hashed %d (model %d)" % (f.arity, len(tid), bad, W.n_bad, hashed, W.n_hashed))
    _same_as_model(out, W)
    assert (bad, hashed) == (W.n_bad, W.n_hashed)
    touched = np.zeros(f.T, dtype=bool)
    touched[list(W.touched)] = True
    _forest_is_the_models(f, trees, untouched_roots=~touched)
    return out, W


# ---- 1. a mixed batch ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_mixed_batch_with_repeated_pairs_matches_one_by_one_application(gpu_ctx, oracle_mod, arity):
    f, trees = _twelve(gpu_ctx, oracle_mod, arity)
    rng = np.random.default_rng(arity)
    k = 701
    tid = np.concatenate([np.arange(len(SIZES)), rng.integers(0, len(SIZES), size=k - len(SIZES))])  # every tree at least once
    lid = (rng.random(k) * np.asarray(SIZES)[tid]).astype(np.int64)
    repeat = rng.random(k) < 1 / 3
    repeat[:len(SIZES)] = False
    for i in np.flatnonzero(repeat):
        j = int(rng.integers(0, i))
        tid[i], lid[i] = tid[j], lid[j]
    shuffle = rng.permutation(k)
    tid, lid = tid[shuffle], lid[shuffle]
    assert k % 256 not in (0, 1) and 200 < int(repeat.sum()) < 270 and set(tid) == set(range(len(SIZES)))
    new = _leaves(k, 5 + arity)
    out, W = _run_against_model(f, trees, oracle_mod, tid, lid, new)
    assert W.n_bad == 0 and W.n_hashed == int(TS.depth(np.asarray(SIZES)[tid], arity).sum())
    back_old, back_new = _rehash(f, out, new)
    assert np.array_equal(back_old, out["before"]) and np.array_equal(back_new, out["after"])  # (these leaves are below p: a one-leaf tree's too)
    # without the optional outputs the rest is the same
    f2, _ = _twelve(gpu_ctx, oracle_mod, arity)
    again, bad, hashed = _call(f2, tid, lid, new, optional=False)
    for name in ("sib", "pos", "dep", "after"):
        assert np.array_equal(again[name], out[name]), name
    assert (again["old"] == SENT64).all() and (again["before"] == SENT64).all() and np.array_equal(f2.state()[2], f2.roots0)
    assert np.array_equal(f2.state()[0], f.state()[0]) and np.array_equal(f2.state()[1], f.state()[1])


# ---- 2. the three extremes of the merge ----
@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("shape", ["one leaf", "one parent", "two ends"])
def test_merge_extremes(gpu_ctx, oracle_mod, arity, shape):
    """300 updates of one leaf (one run all the way up); round-robin over the A leaves of one parent (A runs that merge on level 1);
    alternating between leaf 0 and the last leaf of the 257-leaf tree (two runs that merge only at the root)"""
    f, trees = _twelve(gpu_ctx, oracle_mod, arity)
    k, t = 300, len(SIZES) - 1
    if shape == "one leaf":
        lid = np.full(k, 77)
    elif shape == "one parent":
        lid = 8 * arity + np.arange(k) % arity
    else:
        lid = np.where(np.arange(k) % 2 == 0, 0, SIZES[t] - 1)
    tid = np.full(k, t)
    new = _leaves(k, 300 + arity)
    out, W = _run_against_model(f, trees, oracle_mod, tid, lid, new)
    assert np.array_equal(out["before"][1:], out["after"][:-1]) and np.array_equal(out["before"][0], f.roots0[t])
    if shape == "one leaf":
        assert np.array_equal(out["old"][1:], new[:-1])


# ---- 3. past the lane-group rule ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_batch_past_the_lane_group_rule(gpu_ctx, oracle_mod, arity):
    """k = 8,197 > 8,192: the digests of every level take the one-lane build; a shallow deep tree keeps the model at 4 x 10^4 digests"""
    sizes = [4 ** 5 if arity == 4 else 2 ** 10, 17, 5, 64]
    leaves = _leaves(sum(sizes), 17 * arity)
    f = Forest(gpu_ctx, arity, sizes, leaves)
    f.roots0 = f.state()[2]
    trees = _host_trees(oracle_mod, arity, sizes, leaves, "large")
    rng = np.random.default_rng(30 + arity)
    k = 8197
    tid = rng.choice(len(sizes), size=k, p=[0.4, 0.2, 0.2, 0.2])
    lid = (rng.random(k) * np.asarray(sizes)[tid]).astype(np.int64)
    _run_against_model(f, trees, oracle_mod, tid, lid, _leaves(k, 31 + arity))


# ---- 4. every kind of bad update among good neighbours ----
@pytest.mark.parametrize("arity", [4, 2])
def test_every_kind_of_bad_update_among_good_neighbours(gpu_ctx, oracle_mod, arity):
    sizes = [5, 17, 0, 65, 1, 16]  # tree 2 is empty: bad for whoever names it
    leaves = _leaves(sum(sizes), 23 * arity)
    f = Forest(gpu_ctx, arity, sizes, leaves)
    f.roots0 = f.state()[2]
    trees = _host_trees(oracle_mod, arity, sizes, leaves, "bad tree")
    kinds = [(len(sizes), 0), (2 ** 32 - 1, 3), (2, 0), (1, 17), (3, 2 ** 63), (0, 2 ** 64 - 1), (4, 1)]
    rng = np.random.default_rng(arity)
    good_t = rng.choice([0, 1, 3, 4, 5], size=60)
    good_l = (rng.random(60) * np.asarray(sizes)[good_t]).astype(np.int64)
    tid, lid = [int(x) for x in good_t], [int(x) for x in good_l]
    for at, (t, j) in zip((3, 11, 12, 25, 31, 44, 59), kinds):  # spread among the good ones, two of them neighbours
        tid.insert(at, t), lid.insert(at, j)
    tid, lid = np.array(tid, dtype=np.uint64), np.array(lid, dtype=np.uint64)
    new = _leaves(len(tid), 24 + arity)
    out, W = _run_against_model(f, trees, oracle_mod, tid, lid, new)
    assert W.n_bad == len(kinds) and int((out["dep"] == 0xFF).sum()) == len(kinds)
    for i in np.flatnonzero(out["dep"] == 0xFF):
        assert not (out["old"][i].any() or out["sib"][i].any() or out["pos"][i].any() or out["before"][i].any() or out["after"][i].any())


# ---- 5. every kind of bad order ----
@pytest.mark.parametrize("arity", [4, 2])
def test_every_kind_of_bad_order_refuses_the_batch_and_touches_nothing(gpu_ctx, oracle_mod, arity):
    f, _ = _twelve(gpu_ctx, oracle_mod, arity)
    before = f.state()
    tid = np.array([3, 11, 3, 7, 11, 0, 11, 3, 9, 11])
    lid = np.array([2, 200, 1, 14, 200, 0, 5, 2, 40, 200])
    k = len(tid)
    good = FS.stable_order(tid, lid)
    assert good.tolist() == [5, 2, 0, 7, 3, 8, 6, 1, 4, 9]
    kinds = {"an index twice": [5, 2, 0, 0, 3, 8, 6, 1, 4, 9], "an index = k": [5, 2, 0, 7, 3, 8, 6, 1, 4, k], "an index = 2^32 - 1": [5, 2, 0, 7, 3, 8, 6, 1, 4, 2 ** 32 - 1],
             "trees out of order": [5, 2, 0, 7, 8, 3, 6, 1, 4, 9], "leaves out of order": [5, 0, 2, 7, 3, 8, 6, 1, 4, 9],
             "a tie in descending index": [5, 2, 7, 0, 3, 8, 6, 1, 4, 9], "the last two swapped": [5, 2, 0, 7, 3, 8, 6, 1, 9, 4]}
    new = _leaves(k, 40 + arity)
    for kind, order in kinds.items():
        assert not FS.order_is_valid(order, tid, lid), kind
        out, bad, hashed = _call(f, tid, lid, new, order=order)
        assert (out["dep"] == 0xFF).all() and bad == k and hashed == 0, kind
        for name in ("old", "sib", "before", "after"):
            assert (out[name] == SENT64).all(), (kind, name)
        assert (out["pos"] == 7).all(), kind
        for x, y in zip(f.state(), before):
            assert np.array_equal(x, y), kind
    out, bad, hashed = _call(f, tid, lid, new, order=good)  # the control: the good order applies all ten
    assert bad == 0 and hashed == int(TS.depth(np.asarray(SIZES)[tid], arity).sum()) and (out["dep"] != 0xFF).all()


# ---- 6. distinct pairs ----
@pytest.mark.parametrize("arity", [4, 2])
def test_distinct_pairs_leave_what_update_device_leaves(gpu_ctx, oracle_mod, arity):
    f, _ = _twelve(gpu_ctx, oracle_mod, arity)
    g, _ = _twelve(gpu_ctx, oracle_mod, arity)
    rng = np.random.default_rng(60 + arity)
    pairs = [(t, j) for t, n in enumerate(SIZES) for j in range(n)]
    pick = rng.choice(len(pairs), size=333, replace=False)
    tid, lid = np.array([pairs[i][0] for i in pick]), np.array([pairs[i][1] for i in pick])
    new = _leaves(len(pick), 61 + arity)
    out, bad, hashed = _call(f, tid, lid, new)
    u_bad, u_hashed = _update(gpu_ctx, arity, g.d, g.d_off, g.T, g.top, g.d_lv, tid, lid, new, d_roots=g.d_roots)
    assert bad == 0 == int(u_bad) and hashed >= int(u_hashed) > 0
    for x, y in zip(f.state(), g.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(out["old"], _leaves(sum(SIZES), 91 * arity)[f.off[tid] + lid])  # distinct pairs: every old leaf is the built one


# ---- 7. the modulus edge ----
def _edge_words():
    return np.array([E.limbs(v) for v in (E.P - 1, E.P, E.P + 1, 2 * E.P, 2 * E.P + 5, 2 ** 256 - 1, 2 ** 255, 0)], dtype=np.uint64)


@pytest.mark.parametrize("arity", [4, 2])
def test_leaves_at_and_above_the_modulus_and_one_leaf_trees(gpu_ctx, oracle_mod, arity):
    """old leaves come back byte for byte, roots mod p; a one-leaf tree's root is its leaf mod p"""
    edge = _edge_words()
    sizes = [1, 5, 1, 16, 2]
    leaves = _leaves(sum(sizes), 70 + arity)
    leaves[0], leaves[3], leaves[6] = edge[1], edge[5], edge[3]  # the first one-leaf tree holds p itself
    f = Forest(gpu_ctx, arity, sizes, leaves)
    f.roots0 = f.state()[2]
    trees = FS.build_forest(leaves, sizes, arity, _digest(oracle_mod, arity))
    assert np.array_equal(f.roots0, FS.forest_arrays(trees, E.reduce_mod_p)[2])
    tid = np.array([0, 2, 1, 0, 3, 2, 1, 4, 0, 3, 2, 4, 1, 0, 3, 1])
    lid = np.array([0, 0, 2, 0, 7, 0, 2, 1, 0, 7, 0, 0, 4, 0, 15, 2])
    new = np.concatenate([edge, edge[::-1]])[:len(tid)]
    out, W = _run_against_model(f, trees, oracle_mod, tid, lid, new)
    # update 0 wrote p - 1 and update 3 sees it; update 8 sees 2p of update 3: the bytes as they were written, the root reduced
    assert np.array_equal(out["old"][0], edge[1]) and not out["before"][0].any()
    assert np.array_equal(out["old"][8], new[3]) and np.array_equal(out["before"][8], E.reduce_mod_p(new[3:4])[0]) and not np.array_equal(out["old"][8], out["before"][8])


@pytest.mark.parametrize("arity", [4, 2])
def test_a_forest_of_one_leaf_trees_needs_no_levels(gpu_ctx, oracle_mod, arity):
    """max_leaves == 1: stride 0, d_levels, d_siblings and d_positions are NULL, nothing is hashed"""
    sizes = [1, 1, 1]
    leaves = _leaves(3, 75 + arity)
    f = Forest(gpu_ctx, arity, sizes, leaves)
    f.roots0 = f.state()[2]
    assert f.D == 0
    trees = FS.build_forest(leaves, sizes, arity, _digest(oracle_mod, arity))
    tid, lid = np.array([2, 0, 2, 2, 3, 0, 1]), np.array([0, 0, 0, 0, 0, 1, 0])  # (one unknown tree, one leaf past its tree)
    edge = _edge_words()
    out, W = _run_against_model(f, trees, oracle_mod, tid, lid, edge[:len(tid)])
    assert W.n_hashed == 0 and W.n_bad == 2 and np.array_equal(out["before"][3], out["after"][2])


# ---- 8. two streams ----
@pytest.mark.parametrize("arity", [4, 2])
def test_two_streams_of_one_context_then_trim_give_the_same_bytes(gpu_ctx, oracle_mod, arity):
    import torch
    rng = np.random.default_rng(80 + arity)
    k = 400
    tid = rng.integers(0, len(SIZES), size=k)
    lid = (rng.random(k) * np.asarray(SIZES)[tid]).astype(np.int64) // 3  # (few leaves: many repeats)
    new = _leaves(k, 81 + arity)
    f0, _ = _twelve(gpu_ctx, oracle_mod, arity)
    want, bad, hashed = _call(f0, tid, lid, new)
    results = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for round_ in range(2):
        if round_ == 1:  # the second round starts from cold scratch
            gpu_ctx.trim()
        forests = [_twelve(gpu_ctx, oracle_mod, arity)[0] for _ in range(2)]
        torch.cuda.synchronize()
        launched = []
        for s, f in zip(streams, forests):  # both enqueued before either is read
            with torch.cuda.stream(s):
                launched.append(_launch(f, tid, lid, new))
        results += [(_read(f, b), f.state()) for f, b in zip(forests, launched)]
    for (out, b, h), state in results:
        assert (b, h) == (bad, hashed)
        for name in ("old", "sib", "pos", "dep", "before", "after"):
            assert np.array_equal(out[name], want[name]), name
        for x, y in zip(state, f0.state()):
            assert np.array_equal(x, y)


# ---- 9. the convenience ----
@pytest.mark.parametrize("arity", [4, 2])
def test_the_convenience_sorts_for_itself_and_refuses_ids_outside_the_forest(gpu_ctx, oracle_mod, arity):
    import poseidon252_amd as P
    f, trees = _twelve(gpu_ctx, oracle_mod, arity)
    rng = np.random.default_rng(90 + arity)
    k = 150
    tid = rng.integers(0, len(SIZES), size=k)
    lid = (rng.random(k) * np.asarray(SIZES)[tid]).astype(np.int64) // 2
    new = _leaves(k, 92 + arity)
    W = FS.sequential_model(trees, tid, lid, new, f.top, arity, _digest(oracle_mod, arity), E.reduce_mod_p)
    old, sib, pos, dep, before, after, D = P.forest_ragged_update_sequential(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, tid, lid, new, d_roots=f.d_roots,
                                                                            arity=arity)
    gpu_ctx.sync()
    assert D == f.D
    for got, name in ((old, "old"), (sib, "sib"), (pos, "pos"), (dep, "dep"), (before, "before"), (after, "after")):
        assert np.array_equal(_np(got), getattr(W, name)), name
    _forest_is_the_models(f, trees, untouched_roots=np.array([t not in W.touched for t in range(f.T)]))
    state = f.state()
    for bad_t, bad_l in ((len(SIZES), 0), (-1, 0), (0, f.top), (0, -1)):
        with pytest.raises(ValueError, match="outside the forest"):
            P.forest_ragged_update_sequential(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, [0, bad_t], [0, bad_l], new[:2], arity=arity)
    for x, y in zip(f.state(), state):  # refused before anything was enqueued
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        P.forest_ragged_update_sequential(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, [0], [0], new[:1], arity=3)
    with pytest.raises(ValueError, match="1 tree ids, 2 leaf ids"):
        P.forest_ragged_update_sequential(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, [0], [0, 1], new[:1], arity=arity)


# ---- the C++ mirror ----
def test_cpp_mirror_runs(gpu_ctx, tmp_path, oracle_mod):
    from helpers.percall import build_cpp_mirror, run_cpp_mirror
    assert run_cpp_mirror(build_cpp_mirror("test_forest_sequential_api", tmp_path)).strip().endswith("ok")
