"""Leaves appended to the trees of a forest of trees of different sizes (p252_merkle{4,2}_forest_ragged_append_device_into;
csrc/forest_append.hip) on the GPU.  The reference of every comparison is a fresh merkle_forest_ragged_device build of the new forest
as the numpy model (testsupport/forestappend.py, checked without a GPU) lays it out, plus the oracle on the small trees — never
the append itself: offsets, leaves, levels, roots, the digest count and the bad count; clean nodes moved and not hashed again; refused
appends; both digest kernels and more trees than one scan tile; two appends in a row, openings and updates of the grown forest; two
streams, graph capture, the C++ mirror."""
import numpy as np
import pytest

from testsupport.forestappend import forest_append_model, model_leaves
from helpers.forest import SENTINEL, Grown, Old, _append, _fresh, _np, _open, _outputs, _tag, _torch, _tree, _verify
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048                # FOREST_APPEND_SCAN_TILE of csrc/forest_append.h


def _run(ctx, oracle_mod, arity, flat, off, max_leaves, add, aoff, max_new, oracle_up_to=70):
    """build, append, compare with the fresh build and the model -> (old, model, outputs)"""
    import torch
    n_trees_new = len(aoff) - 1
    old = Old(ctx, arity, flat, off, max_leaves)
    M = forest_append_model(off, flat.shape[0], max_leaves, aoff, add.shape[0], max_new, arity)
    out = _outputs(arity, flat.shape[0] + add.shape[0], n_trees_new, max_new)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_add = _torch(add) if add.shape[0] else None
    _append(ctx, old, d_add, _torch(np.asarray(aoff, np.uint64)), n_trees_new, max_new, out, bad, hashed)
    ref = _fresh(ctx, arity, M, flat, add, n_trees_new, max_new, out)
    torch.cuda.synchronize()
    for name, got, want in zip(("leaves", "offsets", "levels", "roots"), out, ref):  # the sentinel tails included: nothing written past the used lengths
        assert torch.equal(got, want), name
    used = int(M["lo_new"][-1])
    assert bool((out[2][used:] == SENTINEL).all()) and not bool((out[2][:used] == SENTINEL).all(dim=1).any())
    assert int(hashed) == M["n_hashed"] and int(bad) == M["n_bad"], (int(hashed), M["n_hashed"], int(bad), M["n_bad"])
    roots, leaves = _np(out[3]), _np(out[0])
    tree = _tree(oracle_mod, arity)
    for t, n in enumerate(M["n_new"]):
        if n == 0:
            assert not roots[t].any(), t
        elif n <= oracle_up_to:
            at = int(M["offsets_new"][t])
            assert np.array_equal(roots[t], tree(_tag(arity), leaves[at:at + n])[0]), t
    return old, M, out


def _mixed(arity):
    """old sizes and appends: every listed edge among 36 old trees, in a fixed shuffled order, and three brand-new trees"""
    N, Mm = [0, 1, 3, 4, 5, 16, 17, 21, 64], [0, 1, 3, 11, 48, 200]
    pairs = [(n, m) for i, n in enumerate(N) for j, m in enumerate(Mm) if j not in ((i + 1) % 6, (i + 4) % 6)]
    for must in ((0, 0), (0, 3), (1, 48), (1, 1), (4, 200), (16, 1), (64, 3), (5, 0), (5, 1), (17, 0), (21, 11)):
        assert must in pairs
    np.random.default_rng(arity).shuffle(pairs)
    return [p[0] for p in pairs], [p[1] for p in pairs] + [5, 1, 48]


# ---- 1. one mixed forest ----
@pytest.mark.parametrize("arity", [4, 2])
def test_mixed_forest_equals_a_fresh_build(gpu_ctx, oracle_mod, arity):
    sizes, adds = _mixed(arity)
    off = TS.offsets(sizes, start=5)  # offsets[0] != 0
    flat = oracle_mod.fill_random(0xA00 + arity, int(off[-1]) + 3)
    aoff = TS.offsets(adds)
    add = oracle_mod.fill_random(0xA10 + arity, int(aoff[-1]))
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 64, add, aoff, 264)
    assert len(adds) == len(sizes) + 3 and M["n_bad"] == 1 and not any(M["refused"])  # (the tree that stays empty)
    assert M["n_old"][:len(sizes)] == sizes and M["m"] == adds
    assert 0 < M["n_hashed"] < int(M["lo_new"][-1])  # some nodes hashed, not all
    # unchanged trees keep their roots
    for t in range(len(sizes)):
        if adds[t] == 0 and sizes[t]:
            assert np.array_equal(_np(out[3])[t], _np(old.roots)[t]), t


# ---- 2. moved, not hashed again ----
@pytest.mark.parametrize("arity", [4, 2])
def test_clean_nodes_are_moved_and_dirty_ones_hashed_from_what_lies_below(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, adds = _mixed(arity)
    off, aoff = TS.offsets(sizes, start=2), TS.offsets(adds)
    flat = oracle_mod.fill_random(0xA20 + arity, int(off[-1]))
    add = oracle_mod.fill_random(0xA30 + arity, int(aoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 64)
    used_old = sum(sum(TS.level_widths(n, arity)) for n in sizes)
    # junk that no digest equals, one value per slot, each a valid scalar (the top limb is below the modulus')
    junk = np.zeros((old.d_lv.shape[0], 4), dtype=np.uint64)
    junk[:, 0], junk[:, 1], junk[:, 3] = np.arange(1, junk.shape[0] + 1), 0x1111, 0x0123456789ABCDEF
    old.d_lv.copy_(_torch(junk))
    M = forest_append_model(off, flat.shape[0], 64, aoff, add.shape[0], 264, arity)
    out = _outputs(arity, flat.shape[0] + add.shape[0], len(adds), 264)
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _append(gpu_ctx, old, _torch(add), _torch(aoff), len(adds), 264, out, None, hashed)
    torch.cuda.synchronize()
    got, leaves = _np(out[2]), model_leaves(M, flat, add)
    assert np.array_equal(_np(out[0])[:leaves.shape[0]], leaves) and int(hashed) == M["n_hashed"]
    # the expected levels, tree by tree and level by level: junk where clean, the oracle's digest of the expected children where dirty
    want = np.zeros((int(M["lo_new"][-1]), 4), dtype=np.uint64)
    n_clean = 0
    for t, n in enumerate(M["n_new"]):
        below, at = leaves[int(M["offsets_new"][t]):int(M["offsets_new"][t]) + n], int(M["lo_new"][t])
        for w in TS.level_widths(n, arity):
            kids = np.zeros((w * arity, 4), dtype=np.uint64)
            kids[:below.shape[0]] = below
            digests = oracle_mod.hash_batch(_tag(arity), kids.reshape(w, arity, 4), arity, 1).reshape(w, 4)
            src = M["node_src"][at:at + w]
            assert (src[src >= 0] < used_old).all()
            want[at:at + w] = np.where((src >= 0)[:, None], junk[np.maximum(src, 0)], digests)
            n_clean += int((src >= 0).sum())
            below, at = want[at:at + w], at + w
    assert n_clean > 100 and n_clean + M["n_hashed"] == want.shape[0]
    assert np.array_equal(got[:want.shape[0]], want)
    assert bool((out[2][want.shape[0]:] == SENTINEL).all())


# ---- 3. bad appends ----
@pytest.mark.parametrize("arity", [4, 2])
def test_refused_appends_keep_the_tree_and_are_counted_once(gpu_ctx, oracle_mod, arity):
    sizes = [10, 20, 5, 30, 8]
    off = TS.offsets(sizes, start=1)
    flat = oracle_mod.fill_random(0xA40 + arity, int(off[-1]) + 2)
    # tree 1: decreasing offsets; tree 2: accepted (its range overlaps tree 0's); tree 3: 30 + 6 > max_leaves_new; tree 4: past n_add;
    # tree 5 (new): decreasing, and empty as well — counted once
    aoff = np.array([0, 4, 2, 6, 12, 45, 40], dtype=np.uint64)
    add = oracle_mod.fill_random(0xA50 + arity, 40)
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 30, add, aoff, 35)
    assert M["refused"] == [False, True, False, True, True, True] and M["m"] == [4, 0, 4, 0, 0, 0] and M["n_bad"] == 4
    leaves, roots = _np(out[0]), _np(out[3])
    for t in (1, 3, 4):  # the refused trees: their old leaves, their old root
        at = int(M["offsets_new"][t])
        assert np.array_equal(leaves[at:at + sizes[t]], flat[int(off[t]):int(off[t + 1])]) and int(M["offsets_new"][t + 1]) - at == sizes[t]
        assert np.array_equal(roots[t], _np(old.roots)[t])
    assert np.array_equal(leaves[int(M["offsets_new"][2]) + 5:int(M["offsets_new"][3])], add[2:6])
    # ranges that overlap behind a decrease and would take the forest past n_add: the sum rule refuses the later one
    aoff = np.array([0, 30, 10, 40, 40, 40, 40], dtype=np.uint64)
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 30, add, aoff, 64)
    assert M["m"] == [30, 0, 0, 0, 0, 0] and M["refused"] == [False, True, True, False, False, False] and M["n_bad"] == 3


# ---- 4. dispatch and tiles ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_level_too_wide_for_the_lane_groups(gpu_ctx, oracle_mod, arity):
    """2^15 leaves appended to one tree of 2^15 + 7: level 1's dirty list is bounded by more than 8,192 nodes, so k_fu_digest runs;
    the levels above run on the 8-lane kernel"""
    n, m = (1 << 15) + 7, 1 << 15
    assert (m >> (2 if arity == 4 else 1)) + 2 > 8192
    flat, add = oracle_mod.fill_random(0xA60 + arity, n), oracle_mod.fill_random(0xA70 + arity, m)
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, TS.offsets([n]), n, add, TS.offsets([m]), n + m, oracle_up_to=1 << 17)
    assert M["n_hashed"] == sum(-(-(n + m) // arity ** l) - n // arity ** l for l in range(1, len(TS.level_widths(n + m, arity)) + 1))


@pytest.mark.parametrize("arity", [4, 2])
def test_more_trees_than_one_scan_tile(gpu_ctx, oracle_mod, arity):
    rng = np.random.default_rng(arity)
    T = SCAN_TILE + 1
    sizes, adds = rng.integers(1, 6, T).tolist(), rng.integers(0, 4, T).tolist()
    sizes[SCAN_TILE - 1], sizes[SCAN_TILE], adds[SCAN_TILE - 1], adds[SCAN_TILE] = 5, 3, 2, 3  # both sides of the tile's edge grow
    off, aoff = TS.offsets(sizes), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xA80 + arity, int(off[-1])), oracle_mod.fill_random(0xA90 + arity, int(aoff[-1]))
    old, M, out = _run(gpu_ctx, oracle_mod, arity, flat, off, 5, add, aoff, 8, oracle_up_to=0)
    tree, roots, leaves = _tree(oracle_mod, arity), _np(out[3]), _np(out[0])
    for t in (0, 1, SCAN_TILE - 1, SCAN_TILE):
        at = int(M["offsets_new"][t])
        assert np.array_equal(roots[t], tree(_tag(arity), leaves[at:at + M["n_new"][t]])[0]), t


# ---- 5. composition ----
@pytest.mark.parametrize("arity", [4, 2])
def test_two_appends_equal_one_and_the_grown_forest_is_an_ordinary_forest(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 4, 5, 16, 0, 33, 64, 2]
    x, y = [3, 0, 1, 5, 2, 0, 1, 9, 4], [1, 7, 0, 4, 0, 0, 64, 1, 0, 6]  # the first call adds one tree, the second another
    T1, T2 = len(x), len(y)
    off, xoff, yoff = TS.offsets(sizes, start=3), TS.offsets(x), TS.offsets(y)
    flat = oracle_mod.fill_random(0xAA0 + arity, int(off[-1]))
    ax, ay = oracle_mod.fill_random(0xAB0 + arity, int(xoff[-1])), oracle_mod.fill_random(0xAC0 + arity, int(yoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 64)
    out1 = _outputs(arity, flat.shape[0] + ax.shape[0], T1, 80)
    _append(gpu_ctx, old, _torch(ax), _torch(xoff), T1, 80, out1)
    g1 = Grown(arity, out1, T1, 80)
    out2 = _outputs(arity, out1[0].shape[0] + ay.shape[0], T2, 160)
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    _append(gpu_ctx, g1, _torch(ay), _torch(yoff), T2, 160, out2, None, hashed)
    # the concatenation in one call
    both = [(x[t] if t < T1 else 0) + y[t] for t in range(T2)]
    boff = TS.offsets(both)
    ab = np.concatenate([np.concatenate([ax[int(xoff[t]):int(xoff[t + 1])] if t < T1 else ax[:0], ay[int(yoff[t]):int(yoff[t + 1])]]) for t in range(T2)])
    M = forest_append_model(off, flat.shape[0], 64, boff, ab.shape[0], 160, arity)
    out12 = _outputs(arity, flat.shape[0] + ab.shape[0], T2, 160)
    _append(gpu_ctx, old, _torch(ab), _torch(boff), T2, 160, out12)
    ref = _fresh(gpu_ctx, arity, M, flat, ab, T2, 160, out12)
    torch.cuda.synchronize()
    n, used = int(M["offsets_new"][-1]), int(M["lo_new"][-1])
    for got in (out2, out12):
        assert torch.equal(got[0][:n], ref[0][:n]) and torch.equal(got[1][:T2 + 1], ref[1][:T2 + 1])
        assert torch.equal(got[2][:used], ref[2][:used]) and torch.equal(got[3][:T2], ref[3][:T2])
    M2 = forest_append_model(_np(out1[1][:T1 + 1]), out1[0].shape[0], 80, yoff, ay.shape[0], 160, arity)
    assert int(hashed) == M2["n_hashed"]
    # openings out of the grown forest verify against its roots through the existing calls
    g2 = Grown(arity, out2, T2, 160)
    n_new = M["n_new"]
    tid = np.array([t for t in range(T2) if n_new[t]] * 2)
    lid = np.array([0 if i < len(tid) // 2 else n_new[t] - 1 for i, t in enumerate(tid)])  # the first leaf, and the last appended one
    o = _open(gpu_ctx, arity, g2.d, g2.d_off, T2, 160, g2.d_lv, tid, lid)
    ok = _verify(gpu_ctx, arity, o, g2.roots, T2)
    torch.cuda.synchronize()
    assert _np(ok).tolist() == [1] * len(tid) and _np(o["bad"]).tolist() == [0, 0]
    # and leaf updates of it still equal a rebuild
    new = oracle_mod.fill_random(0xAD0 + arity, len(tid))
    gpu_ctx.merkle_forest_ragged_update_device(_tag(arity), g2.d, g2.d_off, T2, 160, g2.d_lv, _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64)),
                                               _torch(new), len(tid), d_roots=g2.roots, arity=arity)
    levels, roots = torch.full_like(g2.d_lv, SENTINEL), torch.full_like(out2[3], SENTINEL)
    gpu_ctx.merkle_forest_ragged_device(_tag(arity), g2.d, g2.d_off, T2, 160, roots[:T2], levels, None, arity=arity)
    torch.cuda.synchronize()
    assert torch.equal(g2.d_lv, levels) and torch.equal(out2[3], roots)


def test_merkle_forest_ragged_append_sizes_and_returns_the_new_forest(gpu_ctx, oracle_mod):
    import torch
    from poseidon252_amd import merkle
    sizes, adds = [3, 1, 17], [2, 0, 5, 4]
    off, aoff = TS.offsets(sizes), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xAE0, int(off[-1])), oracle_mod.fill_random(0xAE1, int(aoff[-1]))
    for arity in (4, 2):
        old = Old(gpu_ctx, arity, flat, off, 17)
        leaves, offsets, levels, roots, bad, hashed = merkle.forest_ragged_append(gpu_ctx, None, old.d, old.d_off, 3, 17, old.d_lv, _torch(add), _torch(aoff),
                                                                                 arity=arity)
        M = forest_append_model(off, flat.shape[0], 17, aoff, add.shape[0], 17 + 11, arity)
        torch.cuda.synchronize()
        assert np.array_equal(_np(leaves), model_leaves(M, flat, add)) and _np(offsets).tolist() == M["offsets_new"].tolist()
        assert int(bad) == 0 and int(hashed) == M["n_hashed"]
        tree = _tree(oracle_mod, arity)
        for t in range(4):
            at = int(M["offsets_new"][t])
            assert np.array_equal(_np(roots)[t], tree(_tag(arity), _np(leaves)[at:at + M["n_new"][t]])[0])
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        merkle.forest_ragged_append(gpu_ctx, None, old.d, old.d_off, 3, 17, old.d_lv, _torch(add), _torch(aoff), arity=3)


# ---- 6. streams and capture ----
def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for j, (arity, sizes) in enumerate(((4, [3000, 7, 900, 1] * 10), (2, [65, 1024, 2, 300] * 10))):
        rng = np.random.default_rng(j)
        adds = rng.integers(0, 400, len(sizes) + 2).tolist()
        off, aoff = TS.offsets(sizes), TS.offsets(adds)
        flat, add = oracle_mod.fill_random(0xAF0 + j, int(off[-1])), oracle_mod.fill_random(0xAF8 + j, int(aoff[-1]))
        old = Old(gpu_ctx, arity, flat, off, max(sizes))
        T, max_new = len(adds), max(sizes) + 400
        M = forest_append_model(off, flat.shape[0], max(sizes), aoff, add.shape[0], max_new, arity)
        out = _outputs(arity, flat.shape[0] + add.shape[0], T, max_new)
        jobs.append(dict(old=old, add=_torch(add), aoff=_torch(aoff), T=T, max_new=max_new, out=out, M=M,
                         ref=_fresh(gpu_ctx, arity, M, flat, add, T, max_new, out), hashed=torch.zeros(1, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for rep in range(4):
        for J, s in zip(jobs, streams):
            with torch.cuda.stream(s):
                for t in J["out"]:
                    t.fill_(SENTINEL)
                J["hashed"].zero_()
                _append(gpu_ctx, J["old"], J["add"], J["aoff"], J["T"], J["max_new"], J["out"], None, J["hashed"])
        torch.cuda.synchronize()
        for J in jobs:
            assert all(torch.equal(g, w) for g, w in zip(J["out"], J["ref"])), (rep, J["old"].arity)
            assert int(J["hashed"]) == J["M"]["n_hashed"], (rep, J["old"].arity)


@pytest.mark.parametrize("arity", [4, 2])
def test_graph_capture_replays_on_new_leaves(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 5, 17, 256, 1000, 3, 64, 0] * 10
    adds = np.random.default_rng(arity).integers(0, 40, len(sizes) + 1).tolist()
    off, aoff = TS.offsets(sizes), TS.offsets(adds)
    flat, add = oracle_mod.fill_random(0xB00 + arity, int(off[-1])), oracle_mod.fill_random(0xB10 + arity, int(aoff[-1]))
    old = Old(gpu_ctx, arity, flat, off, 1000)
    T, max_new = len(adds), 1040
    out = _outputs(arity, flat.shape[0] + add.shape[0], T, max_new)
    d_add, d_aoff = _torch(add), _torch(aoff)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _append(gpu_ctx, old, d_add, d_aoff, T, max_new, out, bad, hashed)  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _append(gpu_ctx, old, d_add, d_aoff, T, max_new, out, bad, hashed)
    add2 = oracle_mod.fill_random(0xB20 + arity, add.shape[0])
    d_add.copy_(_torch(add2))
    for t in out:
        t.fill_(SENTINEL)
    bad.zero_()
    hashed.zero_()
    g.replay()
    torch.cuda.synchronize()
    M = forest_append_model(off, flat.shape[0], 1000, aoff, add.shape[0], max_new, arity)
    ref = _fresh(gpu_ctx, arity, M, flat, add2, T, max_new, out)
    torch.cuda.synchronize()
    assert all(torch.equal(got, want) for got, want in zip(out, ref))
    assert int(bad) == M["n_bad"] and int(hashed) == M["n_hashed"]


# ---- 7. the C++ mirror ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_append_api", tmp_path))
