"""A forest of Merkle trees of different sizes in one call (p252_merkle{4,2}_forest_ragged*, csrc/forest_ragged.hip) on the GPU:
roots and tree-major levels against the oracle's single-tree builder, the single-tree and equal-size forest calls of the library,
bad trees, streams, graph capture, openings of a tree's block, offsets past 4 GiB and the relative speed floors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.forest import _median_ms, _mix, _np, _tag, _torch
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_forest(ctx, arity, d_leaves, d_off, n_trees, max_leaves, levels=False, bad=False, stream=None):
    import torch
    n_leaves = d_leaves.numel() // 4
    roots = torch.full((n_trees, 4), -1, dtype=torch.int64, device=d_leaves.device)
    d_lv = torch.zeros((max(TS.levels_bound(n_leaves, n_trees, max_leaves, arity), 1), 4), dtype=torch.int64,
                       device=d_leaves.device) if levels else None
    d_bad = torch.zeros(1, dtype=torch.int32, device=d_leaves.device) if bad else None
    ctx.merkle_forest_ragged_device(_tag(arity), d_leaves, d_off, n_trees, max_leaves, roots, d_lv, d_bad, arity=arity)
    return roots, d_lv, d_bad


def _single_tree_device(ctx, arity, d_leaves, lo, hi, levels=False):
    """p252_merkle{4,2}_tree_device on one tree of a device leaf buffer"""
    import torch
    from poseidon252_amd import _lib
    from poseidon252_amd.hash import _stream
    import ctypes
    L = _lib.lib()
    n = hi - lo
    root = torch.empty(4, dtype=torch.int64, device=d_leaves.device)
    ll = (L.p252_merkle4_levels_len if arity == 4 else L.p252_merkle2_levels_len)(n)
    lv = torch.empty((max(ll, 1), 4), dtype=torch.int64, device=d_leaves.device) if levels else None
    fn = L.p252_merkle4_tree_device if arity == 4 else L.p252_merkle2_tree_device
    tag = np.ascontiguousarray(_tag(arity), dtype=np.uint64)
    rc = fn(ctx._h, tag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), d_leaves.data_ptr() + lo * 32, n, root.data_ptr(),
            lv.data_ptr() if levels else None, _stream(ctx))
    assert rc == 0, L.p252_last_error(ctx._h)
    return root, (lv[:ll] if levels else None)


@pytest.mark.parametrize("arity", [4, 2])
def test_oracle_parity_roots_and_levels(gpu_ctx, oracle_mod, arity):
    import poseidon252_amd as P
    sizes = _mix(arity) * 2
    np.random.default_rng(arity).shuffle(sizes)
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0xF0 + arity, int(off[-1]))
    tag = _tag(arity)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    roots, levels, lo = P.merkle_forest_ragged((flat, off), arity=arity, ctx=gpu_ctx, want_levels=True)
    assert roots.shape == (len(sizes), 4) and lo.shape == (len(sizes) + 1,) and levels.shape == (int(lo[-1]), 4)
    for t, n in enumerate(sizes):
        r, lv, _ = tree(tag, flat[int(off[t]):int(off[t + 1])], want_levels=True)
        assert np.array_equal(roots[t], r), (arity, t, n)
        assert np.array_equal(levels[int(lo[t]):int(lo[t + 1])], lv), (arity, t, n)
    # the list form and the device form, roots only and with levels
    assert np.array_equal(P.merkle_forest_ragged([flat[int(off[t]):int(off[t + 1])] for t in range(len(sizes))], arity=arity,
                                                 ctx=gpu_ctx), roots)
    d, d_off = _torch(flat), _torch(off)
    r0, _, _ = _device_forest(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
    r1, d_lv, _ = _device_forest(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), levels=True)
    assert np.array_equal(_np(r0), roots) and np.array_equal(_np(r1), roots)
    assert np.array_equal(_np(d_lv)[:int(lo[-1])], levels)


def _big_mix(arity, min_level1, seed):
    base = _mix(arity)
    l1 = sum((n + arity - 1) // arity for n in base if n > 1)
    reps = min_level1 // l1 + 1
    sizes = base * reps
    np.random.default_rng(seed).shuffle(sizes)
    return sizes


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import poseidon252_amd as P
from poseidon252_amd import merkle as M
arity, n_trees, max_leaves = %(arity)d, %(n_trees)d, %(max_leaves)d
flat = np.load(%(flat)r); off = np.load(%(off)r)
d = torch.from_numpy(flat.view(np.int64)).to("cuda:0"); d_off = torch.from_numpy(off.view(np.int64)).to("cuda:0")
ctx = P.Context(0)
roots = torch.empty((n_trees, 4), dtype=torch.int64, device="cuda:0")
tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, max_leaves, roots, arity=arity)
np.save(%(out)r, roots.cpu().numpy())
"""


@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("min_level1", [16385, (1 << 20) + 1])
def test_both_kernel_families_equal_single_tree_calls(gpu_ctx, oracle_mod, tmp_path, arity, min_level1):
    import torch
    sizes = _big_mix(arity, min_level1, seed=min_level1 + arity)
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0xB1 + arity, int(off[-1]))
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv, _ = _device_forest(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), levels=True)
    roots = _np(roots)
    r_only, _, _ = _device_forest(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
    assert np.array_equal(_np(r_only), roots)
    from poseidon252_amd import levels_len
    lo = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum([levels_len(n, arity) for n in sizes], out=lo[1:])
    rng = np.random.default_rng(7)
    sample = sorted(set([0, len(sizes) - 1] + list(rng.choice(len(sizes), 150, replace=False))))
    for t in sample:
        r, lv = _single_tree_device(gpu_ctx, arity, d, int(off[t]), int(off[t + 1]), levels=True)
        assert torch.equal(r, torch.from_numpy(roots[t].view(np.int64)).to(r.device)), (t, sizes[t])
        assert torch.equal(d_lv[int(lo[t]):int(lo[t + 1])], lv[:int(lo[t + 1] - lo[t])]), (t, sizes[t])
    # the one-lane kernel on every level: P252_COOP_MAX_NODES=0 in a fresh process
    np.save(str(tmp_path / "flat.npy"), flat)
    np.save(str(tmp_path / "off.npy"), off)
    code = _CHILD % dict(root=ROOT, arity=arity, n_trees=len(sizes), max_leaves=max(sizes), flat=str(tmp_path / "flat.npy"),
                         off=str(tmp_path / "off.npy"), out=str(tmp_path / "roots.npy"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, P252_COOP_MAX_NODES="0"), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert np.array_equal(np.load(str(tmp_path / "roots.npy")).view(np.uint64), roots)


@pytest.mark.parametrize("arity,k", [(4, 3), (2, 5)])
def test_equal_sizes_equal_the_forest(gpu_ctx, oracle_mod, arity, k):
    import torch
    per, n_trees = arity ** k, 300
    flat = oracle_mod.fill_random(0xE0 + arity, per * n_trees)
    d = _torch(flat)
    exp = torch.empty((n_trees, 4), dtype=torch.int64, device=d.device)
    gpu_ctx.merkle4_forest_device(_tag(arity), d, n_trees, per, exp, arity=arity)
    got, _, _ = _device_forest(gpu_ctx, arity, d, _torch(TS.offsets([per] * n_trees)), n_trees, per)
    assert torch.equal(got, exp)


def test_modes_agree_and_edge_calls(gpu_ctx, oracle_mod):
    import torch
    import poseidon252_amd as P
    sizes = [5, 1, 17, 64, 300, 2]
    off = TS.offsets(sizes, start=3)  # offsets[0] need not be 0
    flat = oracle_mod.fill_random(0xA4, int(off[-1]) + 2)
    host_roots, host_lv, lo = P.merkle_forest_ragged((flat, off), ctx=gpu_ctx, want_levels=True)
    assert np.array_equal(P.merkle_forest_ragged((flat, off), ctx=gpu_ctx), host_roots)
    d, d_off = _torch(flat), _torch(off)
    r0, _, _ = _device_forest(gpu_ctx, 4, d, d_off, len(sizes), 300)
    r1, d_lv, _ = _device_forest(gpu_ctx, 4, d, d_off, len(sizes), 300, levels=True)
    assert np.array_equal(_np(r0), host_roots) and np.array_equal(_np(r1), host_roots)
    assert np.array_equal(_np(d_lv)[:int(lo[-1])], host_lv)
    # n_trees = 0: nothing enqueued, the roots untouched
    keep = torch.full((1, 4), 7, dtype=torch.int64, device=d.device)
    gpu_ctx.merkle_forest_ragged_device(_tag(4), d, d_off, 0, 300, keep)
    assert int(keep.sum()) == 28
    assert P.merkle_forest_ragged([], ctx=gpu_ctx).shape == (0, 4)
    # one tree equals the single-tree call
    r, _ = _single_tree_device(gpu_ctx, 4, d, 3, 3 + 300)
    one, _, _ = _device_forest(gpu_ctx, 4, d, _torch(np.array([3, 303], np.uint64)), 1, 300)
    assert torch.equal(one[0], r)


def test_bad_trees_on_the_device_and_the_host(gpu_ctx, oracle_mod):
    import poseidon252_amd as P
    flat = oracle_mod.fill_random(0xBAD, 1000)
    # max_leaves 300: t1 empty, t3 longer than max_leaves, t5 decreasing offsets, t9 past n_leaves; t6 overlaps t4 and is good
    off = np.array([0, 10, 10, 30, 340, 370, 360, 365, 600, 800, 1010], dtype=np.uint64)
    good = {0: (0, 10), 2: (10, 30), 4: (340, 370), 6: (360, 365), 7: (365, 600), 8: (600, 800)}
    d = _torch(flat)
    roots, d_lv, d_bad = _device_forest(gpu_ctx, 4, d, _torch(off), 10, 300, levels=True, bad=True)
    roots = _np(roots)
    assert int(d_bad.item()) == 4
    for t in (1, 3, 5, 9):
        assert not roots[t].any(), t
    tag = _tag(4)
    lv_all = _np(d_lv)
    at = 0
    for t in sorted(good):
        lo, hi = good[t]
        r, lv, _ = oracle_mod.merkle4_tree(tag, flat[lo:hi], want_levels=True)
        assert np.array_equal(roots[t], r), t
        assert np.array_equal(lv_all[at:at + lv.shape[0]], lv), t  # LO counts good trees only
        at += lv.shape[0]
    # the host form refuses the same kinds before any device work
    for bad_off in ([0, 10, 10], [0, 30, 20, 40]):
        with pytest.raises(ValueError):
            gpu_ctx.merkle_forest_ragged(tag, flat, np.array(bad_off, np.uint64))
    from poseidon252_amd import _lib
    L = _lib.lib()
    import ctypes
    u64p = ctypes.POINTER(ctypes.c_uint64)
    roots_h = np.zeros((2, 4), np.uint64)
    for bad_off in ([0, 10, 10], [0, 30, 20]):
        o = np.array(bad_off, np.uint64)
        rc = L.p252_merkle4_forest_ragged(gpu_ctx._h, tag.ctypes.data_as(u64p), flat.ctypes.data_as(u64p), o.ctypes.data_as(u64p), 2,
                                          roots_h.ctypes.data_as(u64p), None)
        assert rc == _lib.ERR_INVALID_ARGUMENT, rc


def test_device_argument_checks(gpu_ctx):
    import torch
    from poseidon252_amd import _lib
    from poseidon252_amd.hash import _stream
    import ctypes
    L = _lib.lib()
    d = torch.zeros((64, 4), dtype=torch.int64, device="cuda:0")
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device="cuda:0")
    roots = torch.zeros((2, 4), dtype=torch.int64, device="cuda:0")
    bad = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    tag = np.zeros(4, np.uint64)
    tp = tag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    f = L.p252_merkle4_forest_ragged_device
    st = _stream(gpu_ctx)
    E = _lib.ERR_INVALID_ARGUMENT
    assert f(gpu_ctx._h, tp, d.data_ptr(), 64, off.data_ptr(), 2, 0, roots.data_ptr(), None, None, st) == E  # max_leaves 0
    assert f(gpu_ctx._h, tp, None, 64, off.data_ptr(), 2, 8, roots.data_ptr(), None, None, st) == E
    assert f(gpu_ctx._h, tp, d.data_ptr() + 8, 64, off.data_ptr(), 2, 8, roots.data_ptr(), None, None, st) == E
    assert f(gpu_ctx._h, tp, d.data_ptr(), 64, off.data_ptr() + 4, 2, 8, roots.data_ptr(), None, None, st) == E
    assert f(gpu_ctx._h, tp, d.data_ptr(), 64, off.data_ptr(), 2, 8, roots.data_ptr(), None, bad.data_ptr() + 2, st) == E
    assert f(gpu_ctx._h, tp, d.data_ptr(), 1 << 62, off.data_ptr(), 2, 8, roots.data_ptr(), None, None, st) == E  # overflow
    assert f(gpu_ctx._h, tp, None, 0, None, 0, 0, None, None, None, st) == 0  # n_trees = 0
    with pytest.raises(ValueError):  # the binding: a host array is no device buffer
        gpu_ctx.merkle_forest_ragged_device(tag, np.zeros((4, 4), np.uint64), off, 2, 8, roots)


def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    import torch
    import poseidon252_amd as P
    dev = torch.device("cuda:0")
    jobs = []
    for k, sizes in enumerate(([3000, 7, 900, 1] * 40, [65, 4096, 2, 300] * 30)):
        off = TS.offsets(sizes)
        flat = oracle_mod.fill_random(0x5E + k, int(off[-1]))
        jobs.append((sizes, off, flat, _torch(flat), _torch(off)))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = []
    for (sizes, off, flat, d, d_off), s in zip(jobs, streams):
        with torch.cuda.stream(s):
            outs.append(_device_forest(gpu_ctx, 4, d, d_off, len(sizes), max(sizes))[0])
    torch.cuda.synchronize()
    for (sizes, off, flat, d, d_off), got in zip(jobs, outs):
        assert np.array_equal(_np(got), P.merkle_forest_ragged((flat, off), ctx=gpu_ctx))


def test_graph_capture_replays_on_new_leaves(gpu_ctx, oracle_mod):
    import torch
    import poseidon252_amd as P
    sizes = [1, 5, 17, 256, 1000, 3, 64] * 20
    off = TS.offsets(sizes)
    n = int(off[-1])
    d = _torch(oracle_mod.fill_random(0x61, n))
    d_off = _torch(off)
    roots = torch.zeros((len(sizes), 4), dtype=torch.int64, device=d.device)
    tag = _tag(4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu_ctx.merkle_forest_ragged_device(tag, d, d_off, len(sizes), 1000, roots)  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gpu_ctx.merkle_forest_ragged_device(tag, d, d_off, len(sizes), 1000, roots)
    fresh = oracle_mod.fill_random(0x62, n)
    d.copy_(_torch(fresh))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(roots), P.merkle_forest_ragged((fresh, off), ctx=gpu_ctx))


@pytest.mark.parametrize("arity", [4, 2])
def test_tree_block_feeds_openings_and_verify(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [70, 1, 300, 16, 5]
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0x0B + arity, int(off[-1]))
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv, _ = _device_forest(gpu_ctx, arity, d, d_off, len(sizes), 300, levels=True)
    from poseidon252_amd import levels_len
    lo = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum([levels_len(n, arity) for n in sizes], out=lo[1:])
    for t, n in enumerate(sizes):
        if n == 1:
            continue
        leaves_t = d[int(off[t]):int(off[t + 1])]
        idx = torch.arange(n, dtype=torch.int32, device=d.device)
        out, sib, pos, depth = gpu_ctx.merkle4_openings_device(leaves_t, n, d_lv[int(lo[t]):int(lo[t + 1])], idx, n, check=True, arity=arity)
        ok = torch.zeros(n, dtype=torch.uint8, device=d.device)
        gpu_ctx.merkle_verify_batch_device(_tag(arity), out, sib, pos, depth, roots[t], ok, n, arity=arity)
        torch.cuda.synchronize()
        assert int(ok.sum()) == n, (arity, t)


def test_offsets_past_4_gib(gpu_ctx, oracle_mod):
    import torch
    start = (1 << 27) + 3  # more than 2^27 leaves (4 GiB) before the first tree
    sizes = [1, 9, 1000, 64, 4097]
    off = TS.offsets(sizes, start=start)
    d = torch.zeros((int(off[-1]) + 5, 4), dtype=torch.int64, device="cuda:0")
    d[start:int(off[-1])] = _torch(oracle_mod.fill_random(0x64, int(off[-1]) - start))
    roots, _, _ = _device_forest(gpu_ctx, 4, d, _torch(off), len(sizes), 4097)
    for t in range(len(sizes)):
        r, _ = _single_tree_device(gpu_ctx, 4, d, int(off[t]), int(off[t + 1]))
        assert torch.equal(roots[t], r), t
    del d
    torch.cuda.empty_cache()


def test_relative_speed_floors(gpu_ctx):
    import torch
    tag = _tag(4)
    # W1: equal sizes, the ragged call against the equal-size forest, alternated in one process
    n_trees, per = 1024, 4 ** 6
    d = torch.randint(0, 1 << 60, (n_trees * per, 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(TS.offsets([per] * n_trees))
    roots_a = torch.empty((n_trees, 4), dtype=torch.int64, device=d.device)
    roots_b = torch.empty_like(roots_a)
    forest = lambda: gpu_ctx.merkle4_forest_device(tag, d, n_trees, per, roots_a)  # noqa: E731
    ragged = lambda: gpu_ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, per, roots_b)  # noqa: E731
    forest(), ragged()
    tf, tr = [], []
    for _ in range(7):
        tf.append(_median_ms(forest, 1))
        tr.append(_median_ms(ragged, 1))
    assert torch.equal(roots_a, roots_b)
    ratio = float(np.median(tf)) / float(np.median(tr))
    assert ratio >= 0.85, "ragged %.3f ms vs forest %.3f ms" % (np.median(tr), np.median(tf))
    # mixed sizes: one call against one tree call per tree (per tree)
    rng = np.random.default_rng(2)
    sizes = np.exp(rng.uniform(0, np.log(4 ** 5), 2000)).astype(np.int64).clip(1, 4 ** 5).tolist()
    off = TS.offsets(sizes)
    dm = torch.randint(0, 1 << 60, (int(off[-1]), 4), dtype=torch.int64, device="cuda:0")
    dm_off = _torch(off)
    roots_m = torch.empty((len(sizes), 4), dtype=torch.int64, device=dm.device)
    one = lambda: gpu_ctx.merkle_forest_ragged_device(tag, dm, dm_off, len(sizes), max(sizes), roots_m)  # noqa: E731
    one()
    t_one = _median_ms(one, 5) / len(sizes)
    sub = 200
    each = lambda: [_single_tree_device(gpu_ctx, 4, dm, int(off[t]), int(off[t + 1])) for t in range(sub)]  # noqa: E731
    each()
    t_each = _median_ms(each, 3) / sub
    assert t_each / t_one >= 20, "per tree: %.4f ms one call, %.4f ms per-tree calls" % (t_one, t_each)
