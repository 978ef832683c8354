"""A forest of trees of different sizes rolled back, and forward again, in one call
(p252_merkle{4,2}_forest_ragged_resize_device_into; csrc/forest_append.hip) on the GPU.  The reference of every comparison is a fresh
merkle_forest_ragged_device build of the new forest as the numpy model (testsupport/forestappend.py, checked without a GPU)
lays it out, plus the oracle on the small trees — never the resize itself: leaves, offsets, the used levels and the roots byte for
byte, the digest count and the bad count; a pure rollback; clean nodes moved and dirty ones hashed from below; trailing trees dropped;
a dirty list too wide for the lane groups across the scan tiles; composition with the append; openings of the result; graph capture;
the C++ mirror."""
import numpy as np
import pytest

from testsupport.forestappend import KEEP_ALL, forest_append_model, forest_resize_model
from helpers.forest import SENTINEL, Grown, Old, _append, _fresh, _np, _open, _outputs, _tag, _torch, _tree, _verify
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048  # FOREST_APPEND_SCAN_TILE of csrc/forest_append.h


def _keep(values):
    return None if values is None else np.array([int(v) & KEEP_ALL for v in values], dtype=np.uint64)


def _resize(ctx, old, keep, d_add, d_aoff, n_trees_new, max_new, out, bad=None, hashed=None):
    call = ctx.merkle4_forest_ragged_resize_device if old.arity == 4 else ctx.merkle2_forest_ragged_resize_device
    call(_tag(old.arity), old.d, old.d_off, old.n_trees, old.max_leaves, old.d_lv, None if keep is None else _torch(_keep(keep)), d_add, d_aoff,
         n_trees_new, max_new, out[0], out[1][:n_trees_new + 1], out[2], out[3][:n_trees_new], bad, hashed)


def _check(ctx, oracle_mod, old, flat, keep, add, aoff, max_new, out, bad, hashed, oracle_up_to=70):
    """the outputs of a call against the fresh build of the model's forest, the model's counts and the oracle's roots -> model"""
    import torch
    arity, n_trees_new = old.arity, len(aoff) - 1
    M = forest_resize_model(old.off, flat.shape[0], old.max_leaves, keep, aoff, add.shape[0], max_new, arity)
    ref = _fresh(ctx, arity, M, flat, add, n_trees_new, max_new, out)
    torch.cuda.synchronize()
    for name, got, want in zip(("leaves", "offsets", "levels", "roots"), out, ref):  # the sentinel tails included: nothing written past the used lengths
        assert torch.equal(got, want), name
    used = int(M["lo_new"][-1])
    assert bool((out[2][used:] == SENTINEL).all()) and not bool((out[2][:used] == SENTINEL).all(dim=1).any())
    assert bool((out[0][int(M["offsets_new"][-1]):] == SENTINEL).all())
    assert int(hashed) == M["n_hashed"] and int(bad) == M["n_bad"], (int(hashed), M["n_hashed"], int(bad), M["n_bad"])
    roots, leaves = _np(out[3]), _np(out[0])
    tree = _tree(oracle_mod, arity)
    for t, n in enumerate(M["n_new"]):
        if n == 0:
            assert not roots[t].any(), t
        elif n <= oracle_up_to:
            at = int(M["offsets_new"][t])
            assert np.array_equal(roots[t], tree(_tag(arity), leaves[at:at + n])[0]), t
    return M


def _run(ctx, oracle_mod, arity, flat, off, max_leaves, keep, add, aoff, max_new, oracle_up_to=70, old=None):
    """build, resize, compare -> (old, model, outputs)"""
    import torch
    n_trees_new = len(aoff) - 1
    old = old or Old(ctx, arity, flat, off, max_leaves)
    out = _outputs(arity, flat.shape[0] + add.shape[0], n_trees_new, max_new)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _resize(ctx, old, keep, _torch(add) if add.shape[0] else None, _torch(np.asarray(aoff, np.uint64)), n_trees_new, max_new, out, bad, hashed)
    return old, _check(ctx, oracle_mod, old, flat, keep, add, aoff, max_new, out, bad, hashed, oracle_up_to), out


def _mixed(arity):
    """39 old trees — three of every listed size — and one new tree: (sizes, keep, adds).  Every tree takes another kept count (nothing,
    one leaf, all but one, all, more than it has, UINT64_MAX, a multiple of the arity and of its square: levels with no dirty node) and
    another append"""
    A = arity
    sizes = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257] * 3
    keep, adds = [], []
    for i, n in enumerate(sizes):
        r, idx = divmod(i, 13)
        options = [0, 1, max(n - 1, 0), n, n + 3, KEEP_ALL, A * ((n - 1) // A) if n > A else n, A * A * ((n - 1) // (A * A)) if n > A * A else 1]
        keep.append(options[(idx + 3 * r + arity) % 8])
        adds.append([0, 1, 5][(idx + r) % 3])
    return sizes, keep + [7], adds + [5]


# ---- 1. one mixed forest ----
@pytest.mark.parametrize("arity", [4, 2])
def test_mixed_forest_equals_a_fresh_build(gpu_ctx, oracle_mod, arity):
    sizes, keep, adds = _mixed(arity)
    off = TS.offsets(sizes, start=5)  # offsets[0] != 0
    flat = oracle_mod.fill_random(0xC00 + arity, int(off[-1]) + 3)
    aoff = TS.offsets(adds)
    add = oracle_mod.fill_random(0xC10 + arity, int(aoff[-1]))
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 257, keep, add, aoff, 262)
    assert len(sizes) == 39 and M["n_old"] == sizes + [0] and M["m"] == adds and not any(M["refused"])
    k = M["k"]
    # what the forest covers: cut to nothing, to one leaf, by one leaf, kept whole three ways, cut with and without an append, and cuts
    # that leave a level without a dirty node (a multiple of the arity: level 1; of its square: level 2 as well)
    cut = [(n, kt, m) for n, kt, m in zip(M["n_old"], k, adds) if kt < n]
    assert any(kt == 0 for _, kt, _ in cut) and any(kt == 1 for n, kt, _ in cut if n > 2) and any(kt == n - 1 for n, kt, _ in cut if n > 2)
    assert any(m == 0 for _, _, m in cut) and any(m == 1 for _, _, m in cut) and any(m == 5 for _, _, m in cut) and len(cut) >= 12
    assert any(kt % arity == 0 and kt >= arity and m == 0 for _, kt, m in cut) and any(kt % arity ** 2 == 0 and kt >= arity ** 2 for _, kt, _ in cut)
    assert sum(1 for v, n in zip(keep, sizes) if v == KEEP_ALL and n) >= 2 and sum(1 for v, n in zip(keep, sizes) if v == n + 3) >= 2
    assert M["n_bad"] == sum(1 for n in M["n_new"] if n == 0) >= 1
    assert 0 < M["n_hashed"] < int(M["lo_new"][-1])  # some nodes hashed, not all
    for t, n in enumerate(sizes):  # unchanged trees keep their roots
        if k[t] == n and adds[t] == 0 and n:
            assert np.array_equal(_np(out[3])[t], _np(old.roots)[t]), t


# ---- 2. nothing appended ----
@pytest.mark.parametrize("arity", [4, 2])
def test_pure_rollback_hashes_at_most_one_node_per_tree_and_level(gpu_ctx, oracle_mod, arity):
    """n_add == 0 and d_add == NULL: the case an append launcher returns early on"""
    sizes = [300, 17, 64, 5, 1, 16, 2, 1000, 33]
    keep = [299, 16, 64, 1, 1, 4, 0, 257, KEEP_ALL]  # (16 of 17, 4 of 16: the root of the cut tree is a clean node for arity 4 and 2)
    off = TS.offsets(sizes, start=1)
    flat = oracle_mod.fill_random(0xC20 + arity, int(off[-1]))
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 1000, keep, flat[:0], np.zeros(len(sizes) + 1, np.uint64), 1000, oracle_up_to=300)
    assert M["m"] == [0] * 9 and M["k"] == [299, 16, 64, 1, 1, 4, 0, 257, 33] and M["n_bad"] == 1
    assert 0 < M["n_hashed"] <= sum(TS.depth(n, arity) for n in M["n_new"])
    assert all(len({t for t, _ in nodes}) == len(nodes) for nodes in M["dirty"].values())  # one node per tree and level at the most
    for t in (2, 4, 8):  # the trees kept whole keep their roots
        assert np.array_equal(_np(out[3])[t], _np(old.roots)[t]), t


# ---- 3. moved, not hashed again; hashed, not moved ----
@pytest.mark.parametrize("arity", [4, 2])
def test_clean_nodes_are_moved_and_dirty_ones_hashed_from_what_lies_below(gpu_ctx, oracle_mod, arity):
    """everything of the old forest that the rule calls dead — the leaves at or past k, the nodes (l, j >= floor(k / A^l)) of every tree
    that changes — is overwritten before the call; the result still equals the fresh build"""
    import torch
    sizes, keep, adds = _mixed(arity)
    off, aoff = TS.offsets(sizes, start=2), TS.offsets(adds)
    flat = oracle_mod.fill_random(0xC30 + arity, int(off[-1]))
    add = oracle_mod.fill_random(0xC40 + arity, int(aoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 257)
    M = forest_resize_model(off, flat.shape[0], 257, keep, aoff, add.shape[0], 262, arity)
    # junk that no digest equals, one value per slot, each a valid scalar (the top limb is below the modulus')
    junk = lambda rows, salt: np.stack([np.arange(1, rows + 1, dtype=np.uint64), np.full(rows, salt, np.uint64), np.zeros(rows, np.uint64),  # noqa: E731
                                        np.full(rows, 0x0123456789ABCDEF, np.uint64)], axis=1)
    leaves, levels = flat.copy(), _np(old.d_lv).copy()
    junk_leaves, junk_levels = junk(leaves.shape[0], 0x1111), junk(levels.shape[0], 0x2222)
    n_dead = 0
    for t, n in enumerate(sizes):
        k = M["k"][t]
        if k == n and M["m"][t] == 0:
            continue  # an unchanged tree is moved whole
        lo = int(off[t])
        leaves[lo + k:lo + n] = junk_leaves[lo + k:lo + n]
        at = int(M["lo_old"][t])
        for l, w in enumerate(TS.level_widths(n, arity), 1):
            first = k // arity ** l
            levels[at + first:at + w] = junk_levels[at + first:at + w]
            n_dead += w - first
            at += w
    assert n_dead > 60
    old.d.copy_(_torch(leaves))
    old.d_lv.copy_(_torch(levels))
    out = _outputs(arity, flat.shape[0] + add.shape[0], len(adds), 262)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _resize(gpu_ctx, old, keep, _torch(add), _torch(aoff), len(adds), 262, out, bad, hashed)
    _check(gpu_ctx, oracle_mod, old, flat, keep, add, aoff, 262, out, bad, hashed)  # (flat: the leaves before the poison)
    # and the other way round: a clean node is the old forest's, not a digest — junk in a clean slot arrives as junk
    t = max(range(len(sizes)), key=lambda i: M["k"][i])  # (a tree that keeps a whole first parent)
    assert M["k"][t] >= arity
    slot = int(M["lo_old"][t])  # node (1, 0) of that tree
    levels[slot] = junk_levels[slot]
    old.d_lv.copy_(_torch(levels))
    _resize(gpu_ctx, old, keep, _torch(add), _torch(aoff), len(adds), 262, out)
    torch.cuda.synchronize()
    assert np.array_equal(_np(out[2])[int(M["lo_new"][t])], junk_levels[slot])


# ---- 4. fewer trees ----
@pytest.mark.parametrize("arity", [4, 2])
def test_trailing_trees_are_dropped(gpu_ctx, oracle_mod, arity):
    sizes = [5, 64, 1, 17, 300, 2, 40]
    off = TS.offsets(sizes, start=3)
    flat = oracle_mod.fill_random(0xC50 + arity, int(off[-1]))
    # nothing else: the survivors unchanged, no digest
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 300, None, flat[:0], np.zeros(5, np.uint64), 300)
    assert M["n_new"] == sizes[:4] and M["n_hashed"] == 0 and M["n_bad"] == 0
    assert np.array_equal(_np(out[3])[:4], _np(old.roots)[:4])
    # dropped while new leaves go to the survivors, one of them cut
    adds = [2, 0, 7, 1, 9]
    aoff = TS.offsets(adds)
    add = oracle_mod.fill_random(0xC60 + arity, int(aoff[-1]))
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 300, [KEEP_ALL, 60, 1, 17, 256], add, aoff, 300, oracle_up_to=300, old=old)
    assert M["n_new"] == [7, 60, 8, 18, 265] and M["n_bad"] == 0
    # down to one tree
    _run(gpu_ctx, oracle_mod, arity, flat, off, 300, [3], flat[:0], np.zeros(2, np.uint64), 300, old=old)


# ---- 5. dispatch and tiles ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_wide_dirty_level_across_the_scan_tiles(gpu_ctx, oracle_mod, arity):
    """8,300 trees of 5 leaves cut to 3: more trees than four scan tiles; level 1's dirty list — one node per tree, bounded by
    2 n_trees_new = 16,600 > 8,192 nodes, so k_fu_digest runs, not the 8-lane kernel — spans every tile boundary"""
    T = 8300
    assert T > 4 * SCAN_TILE and 2 * T > 8192
    off = TS.offsets([5] * T)
    flat = oracle_mod.fill_random(0xC70 + arity, 5 * T)
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 5, [3] * T, flat[:0], np.zeros(T + 1, np.uint64), 5, oracle_up_to=0)
    assert M["n_hashed"] == T * (1 if arity == 4 else 2) and [t for t, _ in M["dirty"][1]] == list(range(T))
    tree, roots = _tree(oracle_mod, arity), _np(out[3])
    for t in (0, SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE, T - 1):
        assert np.array_equal(roots[t], tree(_tag(arity), flat[5 * t:5 * t + 3])[0]), t


# ---- 6. composition ----
@pytest.mark.parametrize("arity", [4, 2])
def test_one_call_equals_resize_then_append_and_an_append_is_undone(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 4, 5, 16, 0, 33, 64, 2, 257]
    keep = [1, 2, 5, 4, 0, 32, 63, 0, 100]
    adds = [3, 0, 1, 5, 2, 0, 1, 9, 4, 6]  # (the tenth tree is new)
    T, T2 = len(sizes), len(adds)
    off, aoff = TS.offsets(sizes, start=3), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xC80 + arity, int(off[-1])), oracle_mod.fill_random(0xC90 + arity, int(aoff[-1]))
    old, M, one = _run(gpu_ctx, oracle_mod, arity, flat, off, 257, keep + [0], add, aoff, 300)
    # the same in two calls: cut, then append to the result
    cut = _outputs(arity, flat.shape[0], T, 257)
    _resize(gpu_ctx, old, keep, None, _torch(np.zeros(T + 1, np.uint64)), T, 257, cut)
    two = _outputs(arity, cut[0].shape[0] + add.shape[0], T2, 300)
    _append(gpu_ctx, Grown(arity, cut, T, 257), _torch(add), _torch(aoff), T2, 300, two)
    torch.cuda.synchronize()
    n, used = int(M["offsets_new"][-1]), int(M["lo_new"][-1])
    assert torch.equal(two[0][:n], one[0][:n]) and torch.equal(two[1][:T2 + 1], one[1][:T2 + 1])
    assert torch.equal(two[2][:used], one[2][:used]) and torch.equal(two[3][:T2], one[3][:T2])
    # append(m), then resize(keep = the old n): the original forest again, levels included
    grown = _outputs(arity, flat.shape[0] + add.shape[0], T2, 300)
    _append(gpu_ctx, old, _torch(add), _torch(aoff), T2, 300, grown)
    back = _outputs(arity, grown[0].shape[0], T, 300)
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _resize(gpu_ctx, Grown(arity, grown, T2, 300), sizes, None, _torch(np.zeros(T + 1, np.uint64)), T, 300, back, None, hashed)
    torch.cuda.synchronize()
    A = forest_append_model(off, flat.shape[0], 257, aoff, add.shape[0], 300, arity)
    B = forest_resize_model(A["offsets_new"], grown[0].shape[0], 300, sizes, np.zeros(T + 1, np.uint64), 0, 300, arity)
    assert B["n_new"] == sizes and int(hashed) == B["n_hashed"] > 0
    n, used = int(off[-1] - off[0]), int(A["lo_old"][-1])
    assert np.array_equal(_np(back[0])[:n], flat[int(off[0]):]) and _np(back[1])[:T + 1].tolist() == (off - off[0]).tolist()
    assert torch.equal(back[2][:used], old.d_lv[:used]) and torch.equal(back[3][:T], old.roots) and bool((back[2][used:] == SENTINEL).all())


# ---- 7. the result is an ordinary forest ----
@pytest.mark.parametrize("arity", [4, 2])
def test_openings_of_the_resized_forest_verify(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import merkle
    sizes, keep, adds = [40, 7, 1, 100, 16], [33, 7, 1, 16, 0], [0, 2, 0, 0, 3]
    off, aoff = TS.offsets(sizes), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xCA0 + arity, int(off[-1])), oracle_mod.fill_random(0xCB0 + arity, int(aoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 100)
    leaves, offsets, levels, roots, bad, hashed = merkle.forest_ragged_resize(gpu_ctx, None, old.d, old.d_off, 5, 100, old.d_lv, _torch(_keep(keep)),
                                                                             _torch(add), _torch(aoff), arity=arity)
    M = forest_resize_model(off, flat.shape[0], 100, keep, aoff, add.shape[0], 100 + 5, arity)
    n_new = M["n_new"]
    assert n_new == [33, 9, 1, 16, 3] and _np(offsets).tolist() == M["offsets_new"].tolist() and int(bad) == 0 and int(hashed) == M["n_hashed"]
    tid = np.array([0, 0, 1, 1, 2, 3, 3, 4])
    lid = np.array([0, 32, 6, 8, 0, 0, 15, 2])  # the first leaf, the last kept one, the last appended one
    o = _open(gpu_ctx, arity, leaves, offsets, 5, 105, levels, tid, lid)
    ok = _verify(gpu_ctx, arity, o, roots, 5)
    torch.cuda.synchronize()
    assert _np(ok).tolist() == [1] * len(tid) and _np(o["bad"]).tolist() == [0, 0]
    # the high-level call with nothing but a kept count, and with nothing at all (a compaction copy)
    leaves, offsets, levels, roots, bad, hashed = merkle.forest_ragged_resize(gpu_ctx, None, old.d, old.d_off, 5, 100, old.d_lv, _torch(_keep([8, 8])), arity=arity)
    assert _np(offsets).tolist() == [0, 8, 15] and roots.shape[0] == 2 and int(bad) == 0
    assert np.array_equal(_np(roots)[0], _tree(oracle_mod, arity)(_tag(arity), flat[:8])[0]) and np.array_equal(_np(roots)[1], _np(old.roots)[1])
    leaves, offsets, levels, roots, bad, hashed = merkle.forest_ragged_resize(gpu_ctx, None, old.d, old.d_off, 5, 100, old.d_lv, arity=arity)
    assert torch.equal(roots, old.roots) and int(hashed) == 0
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        merkle.forest_ragged_resize(gpu_ctx, None, old.d, old.d_off, 5, 100, old.d_lv, arity=3)


# ---- 8. capture ----
def test_graph_capture_replays_on_new_leaves_and_new_kept_counts(gpu_ctx, oracle_mod):
    import torch
    arity = 4
    sizes = [1, 5, 17, 256, 1000, 3, 64, 0] * 10
    rng = np.random.default_rng(11)
    adds = rng.integers(0, 40, len(sizes) + 1).tolist()
    keep1 = [int(rng.integers(0, n + 2)) for n in sizes] + [0]
    keep2 = [int(rng.integers(0, n + 2)) for n in sizes] + [0]
    off, aoff = TS.offsets(sizes), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xCC0, int(off[-1])), oracle_mod.fill_random(0xCC1, int(aoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 1000)
    T, max_new = len(adds), 1040
    out = _outputs(arity, flat.shape[0] + add.shape[0], T, max_new)
    d_add, d_aoff, d_keep = _torch(add), _torch(aoff), _torch(_keep(keep1))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    call = lambda: gpu_ctx.merkle4_forest_ragged_resize_device(_tag(arity), old.d, old.d_off, old.n_trees, 1000, old.d_lv, d_keep, d_add, d_aoff, T,  # noqa: E731
                                                               max_new, out[0], out[1][:T + 1], out[2], out[3][:T], bad, hashed)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    add2 = oracle_mod.fill_random(0xCC2, add.shape[0])
    d_add.copy_(_torch(add2))
    d_keep.copy_(_torch(_keep(keep2)))
    for t in out:
        t.fill_(SENTINEL)
    bad.zero_()
    hashed.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check(gpu_ctx, oracle_mod, old, flat, keep2, add2, aoff, max_new, out, bad, hashed)


# ---- 9. the C++ mirror ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_resize_api", tmp_path))
