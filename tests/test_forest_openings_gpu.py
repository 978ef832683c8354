"""Openings out of a forest of trees of different sizes in one call (p252_merkle{4,2}_forest_ragged_openings_device,
p252_merkle{4,2}_path_ragged_device, p252_merkle{4,2}_forest_ragged_verify_device; csrc/forest_openings.hip) on the GPU: every leaf of
every tree against the numpy cut of the oracle's levels, the re-hash against the oracle's roots, the library's own single-tree
and fixed-depth calls, bad openings, edge sizes, streams, graph capture, a leaf buffer past 4 GiB, p252_trim and the speed floors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.forest import _build, _median_ms, _mix, _np, _open, _tag, _torch, _v2_rate, _verify
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 0xFF


def _merkle2_openings(leaves, levels, indices):
    """the arity-2 twin of merkle.merkle4_openings: one sibling per level, positions in 0..1; missing siblings = zero"""
    per_level, cnt, off = [leaves], leaves.shape[0], 0
    while cnt > 1:
        cnt = (cnt + 1) // 2
        per_level.append(levels[off:off + cnt])
        off += cnt
    depth = len(per_level) - 1
    idx = np.asarray(indices, dtype=np.int64)
    sib = np.zeros((idx.shape[0], depth, 1, 4), dtype=np.uint64)
    pos = np.zeros((idx.shape[0], depth), dtype=np.uint8)
    cur = idx.copy()
    for l in range(depth):
        nodes = per_level[l]
        pos[:, l] = cur & 1
        other = cur ^ 1
        have = other < nodes.shape[0]
        sib[have, l, 0] = nodes[other[have]]
        cur = cur >> 1
    return sib, pos


def _expected(oracle_mod, arity, flat, off, sizes, tree_ids, leaf_ids, D):
    """the numpy cut of the oracle's levels, tree by tree -> (leaves, siblings, positions, depths, roots of the trees)"""
    from poseidon252_amd import merkle as M
    tag = _tag(arity)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    k = len(tree_ids)
    e_leaf = np.zeros((k, 4), np.uint64)
    e_sib = np.zeros((k, D, arity - 1, 4), np.uint64)
    e_pos = np.zeros((k, D), np.uint8)
    e_dep = np.zeros(k, np.uint8)
    roots = np.zeros((len(sizes), 4), np.uint64)
    tree_ids, leaf_ids = np.asarray(tree_ids, np.int64), np.asarray(leaf_ids, np.int64)
    for t, n in enumerate(sizes):
        lv_t = flat[int(off[t]):int(off[t + 1])]
        r, lv, _ = tree(tag, lv_t, want_levels=True)
        roots[t] = r
        sel = np.nonzero(tree_ids == t)[0]
        if not sel.size:
            continue
        s, p = (M.merkle4_openings(lv_t, lv, leaf_ids[sel]) if arity == 4 else _merkle2_openings(lv_t, lv, leaf_ids[sel]))
        d = TS.depth(n, arity)
        assert s.shape[1] == d
        e_leaf[sel] = lv_t[leaf_ids[sel]]
        e_sib[sel, :d] = s.reshape(sel.size, d, arity - 1, 4)
        e_pos[sel, :d] = p
        e_dep[sel] = d
    return e_leaf, e_sib, e_pos, e_dep, roots


def _every_leaf(sizes, seed):
    tid = np.repeat(np.arange(len(sizes)), sizes)
    lid = np.concatenate([np.arange(n) for n in sizes])
    perm = np.random.default_rng(seed).permutation(tid.size)
    return tid[perm], lid[perm]


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import poseidon252_amd as P
from helpers import forest as T
z = np.load(%(inp)r)
arity, sizes = int(z["arity"]), z["sizes"].tolist()
ctx = P.Context(0)
d, d_off = T._torch(z["flat"]), T._torch(z["off"])
roots, d_lv = T._build(ctx, arity, d, d_off, len(sizes), max(sizes))
o = T._open(ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, z["tid"], z["lid"])
ok = T._verify(ctx, arity, o, roots, len(sizes))
torch.cuda.synchronize()
np.savez(%(out)r, sib=T._np(o["sib"]), pos=T._np(o["pos"]), dep=T._np(o["dep"]), back=T._np(o["back"]), ok=T._np(ok), bad=T._np(o["bad"]))
"""


@pytest.mark.parametrize("arity", [4, 2])
def test_oracle_parity_every_leaf_of_every_tree(gpu_ctx, oracle_mod, tmp_path, arity):
    import torch
    sizes = _mix(arity) * 2
    np.random.default_rng(arity).shuffle(sizes)
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0x0F0 + arity, int(off[-1]))
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
    tid, lid = _every_leaf(sizes, 11 + arity)
    o = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid)
    ok = _verify(gpu_ctx, arity, o, roots, len(sizes))
    torch.cuda.synchronize()
    D = o["D"]
    assert D == TS.depth(max(sizes), arity)
    e_leaf, e_sib, e_pos, e_dep, e_roots = _expected(oracle_mod, arity, flat, off, sizes, tid, lid, D)
    assert np.array_equal(_np(roots), e_roots)
    assert np.array_equal(_np(o["leaves"]), e_leaf)
    assert np.array_equal(_np(o["dep"]), e_dep)
    assert np.array_equal(_np(o["pos"]), e_pos)  # (rows at or past the depth: zero)
    assert np.array_equal(_np(o["sib"]), e_sib)
    assert np.array_equal(_np(o["back"]), e_roots[tid])  # the oracle's root of tree tree_ids[i], bit-exact
    assert _np(ok).tolist() == [1] * len(tid)
    assert _np(o["bad"]).tolist() == [0, 0]
    # the identity order: P252_RAGGED_SORT=0 in a fresh process
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, arity=arity, sizes=np.asarray(sizes), flat=flat, off=off, tid=tid, lid=lid)
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), inp=inp, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, P252_RAGGED_SORT="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["sib"], e_sib) and np.array_equal(z["pos"], e_pos) and np.array_equal(z["dep"], e_dep)
    assert np.array_equal(z["back"], e_roots[tid]) and z["ok"].tolist() == [1] * len(tid) and z["bad"].tolist() == [0, 0]


@pytest.mark.parametrize("arity", [4, 2])
def test_rows_equal_the_single_tree_openings_call(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import levels_len
    sizes = _mix(arity)
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0x51 + arity, int(off[-1]))
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
    tid = np.repeat(np.arange(len(sizes)), sizes)
    lid = np.concatenate([np.arange(n) for n in sizes])
    o = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid)
    lo = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum([levels_len(n, arity) for n in sizes], out=lo[1:])
    for t, n in enumerate(sizes):
        a, b = int(off[t]), int(off[t + 1])
        idx = torch.arange(n, dtype=torch.int32, device=d.device)
        lv_t = d_lv[int(lo[t]):int(lo[t + 1])] if n > 1 else None
        out, sib, pos, depth = gpu_ctx.merkle4_openings_device(d[a:b], n, lv_t, idx, n, check=True, arity=arity)
        assert depth == TS.depth(n, arity) and bool((o["dep"][a:b] == depth).all())
        assert torch.equal(o["leaves"][a:b], out)
        assert torch.equal(o["sib"][a:b, :depth], sib) and torch.equal(o["pos"][a:b, :depth], pos)
        assert not bool(o["sib"][a:b, depth:].any()) and not bool(o["pos"][a:b, depth:].any())


@pytest.mark.parametrize("arity,per", [(4, 4 ** 3), (2, 2 ** 6)])
def test_equal_depths_equal_path_batch_device(gpu_ctx, oracle_mod, arity, per):
    import torch
    n_trees, k = 300, 20000
    flat = oracle_mod.fill_random(0xE7 + arity, per * n_trees)
    d, d_off = _torch(flat), _torch(TS.offsets([per] * n_trees))
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, n_trees, per)
    rng = np.random.default_rng(5)
    tid, lid = rng.integers(0, n_trees, k), rng.integers(0, per, k)
    o = _open(gpu_ctx, arity, d, d_off, n_trees, per, d_lv, tid, lid)
    D = o["D"]
    assert bool((o["dep"] == D).all())
    exp = torch.empty((k, 4), dtype=torch.int64, device=d.device)
    fixed = gpu_ctx.merkle4_path_batch_device if arity == 4 else gpu_ctx.merkle2_path_batch_device
    fixed(_tag(arity), o["leaves"], o["sib"], o["pos"], D, exp, k)
    torch.cuda.synchronize()
    assert torch.equal(o["back"], exp)
    assert torch.equal(exp, roots[_torch(np.asarray(tid, np.int64))])


@pytest.mark.parametrize("arity", [4, 2])
def test_negatives(gpu_ctx, oracle_mod, arity):
    """(every bad input here is one the kernels are specified to bound-check)"""
    import torch
    flat = oracle_mod.fill_random(0xBAD + arity, 1000)
    # max_leaves 300: t1 empty, t3 longer than max_leaves, t5 behind decreasing offsets, t9 past n_leaves; t6 overlaps t4 and is good
    off = np.array([0, 10, 10, 30, 340, 370, 360, 365, 600, 800, 1010], dtype=np.uint64)
    good = {0: (0, 10), 2: (10, 30), 4: (340, 370), 6: (360, 365), 7: (365, 600), 8: (600, 800)}
    n_trees, max_leaves = 10, 300
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, n_trees, max_leaves)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    e_roots = {t: tree(_tag(arity), flat[a:b])[0] for t, (a, b) in good.items()}
    # good openings, then: tree id >= n_trees (twice), leaf id >= n_t, an empty tree, a too-long tree, a tree behind decreasing offsets,
    # a tree past n_leaves, a huge leaf id
    g_tid = [0, 2, 4, 6, 7, 7, 7, 7, 8, 8, 0, 2]
    g_lid = [9, 0, 29, 4, 0, 100, 234, 77, 199, 5, 0, 19]
    b_tid = [10, 0x7fffffff, 0, 1, 3, 5, 9, 7]
    b_lid = [0, 0, 10, 0, 0, 0, 0, 1 << 40]
    tid, lid = np.array(g_tid + b_tid), np.array(g_lid + b_lid)
    ng, nb = len(g_tid), len(b_tid)
    o = _open(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid)
    ok = _verify(gpu_ctx, arity, o, roots, n_trees)
    torch.cuda.synchronize()
    assert _np(o["bad"]).tolist() == [nb, nb]  # counted once by the extraction, and once by the re-hash
    dep = _np(o["dep"])
    assert dep[ng:].tolist() == [BAD] * nb and dep[:ng].tolist() == [TS.depth(good[t][1] - good[t][0], arity) for t in g_tid]
    for key in ("leaves", "sib", "pos", "back"):
        assert not _np(o[key])[ng:].any(), key
    assert _np(ok).tolist() == [1] * ng + [0] * nb
    back = _np(o["back"])
    for i, t in enumerate(g_tid):
        assert np.array_equal(back[i], e_roots[t]), (i, t)
        assert np.array_equal(_np(o["leaves"])[i], flat[good[t][0] + g_lid[i]])
    # one flipped limb of a sibling (opening 4), of a leaf (5), one position (6), another tree's id (7): exactly those fail
    o["sib"][4, 0, 0, 1] ^= 1
    o["leaves"][5, 3] ^= 1 << 20
    o["pos"][6, 1] = (o["pos"][6, 1] + 1) % arity
    o["d_tid"][7] = 8
    ok = _verify(gpu_ctx, arity, o, roots, n_trees)
    torch.cuda.synchronize()
    exp_ok = [1] * ng + [0] * nb
    for i in (4, 5, 6, 7):
        exp_ok[i] = 0
    assert _np(ok).tolist() == exp_ok


@pytest.mark.parametrize("arity", [4, 2])
def test_edge_sizes(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import _lib
    # D == 0: every tree a single leaf, no levels at all
    n_trees = 50
    flat = oracle_mod.fill_random(0xD0 + arity, n_trees)
    d, d_off = _torch(flat), _torch(TS.offsets([1] * n_trees))
    roots = torch.zeros((n_trees, 4), dtype=torch.int64, device=d.device)
    gpu_ctx.merkle_forest_ragged_device(_tag(arity), d, d_off, n_trees, 1, roots, None, None, arity=arity)
    tid = np.array([3, 49, 0, 50, 3])
    o = _open(gpu_ctx, arity, d, d_off, n_trees, 1, None, tid, np.array([0, 0, 0, 0, 1]))
    ok = _verify(gpu_ctx, arity, o, roots, n_trees)
    torch.cuda.synchronize()
    assert o["D"] == 0 and _np(o["dep"]).tolist() == [0, 0, 0, BAD, BAD] and _np(o["bad"]).tolist() == [2, 2]
    assert np.array_equal(_np(o["leaves"])[:3], flat[[3, 49, 0]]) and not _np(o["leaves"])[3:].any()
    assert np.array_equal(_np(o["back"])[:3], flat[[3, 49, 0]]) and not _np(o["back"])[3:].any()
    assert _np(ok).tolist() == [1, 1, 1, 0, 0]
    # a mixed forest: k = 0 (nothing enqueued, the C call takes NULL buffers), k = 1, k = 70,000 (several sort tiles)
    sizes = _mix(arity) * 2
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0xD1 + arity, int(off[-1]))
    d, d_off = _torch(flat), _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    e_roots = np.stack([tree(_tag(arity), flat[int(off[t]):int(off[t + 1])])[0] for t in range(len(sizes))])
    L = _lib.lib()
    fn = L.p252_merkle4_forest_ragged_openings_device if arity == 4 else L.p252_merkle2_forest_ragged_openings_device
    assert fn(gpu_ctx._h, None, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None) == 0
    o0 = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert o0["leaves"].shape[0] == 0
    rng = np.random.default_rng(70 + arity)
    for k in (1, 70000):
        tid = rng.integers(0, len(sizes), k)
        lid = (rng.random(k) * np.asarray(sizes)[tid]).astype(np.int64)
        o = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid)
        ok = _verify(gpu_ctx, arity, o, roots, len(sizes))
        torch.cuda.synchronize()
        assert np.array_equal(_np(o["back"]), e_roots[tid]), k
        assert np.array_equal(_np(o["leaves"]), flat[off[tid].astype(np.int64) + lid]), k
        assert int(ok.sum()) == k and _np(o["bad"]).tolist() == [0, 0]


def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for j, (arity, sizes) in enumerate(((4, [3000, 7, 900, 1] * 10), (2, [65, 1024, 2, 300] * 10))):
        off = TS.offsets(sizes)
        flat = oracle_mod.fill_random(0x5E0 + j, int(off[-1]))
        d, d_off = _torch(flat), _torch(off)
        roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), max(sizes))
        rng = np.random.default_rng(j)
        tid = rng.integers(0, len(sizes), 30000)
        lid = (rng.random(30000) * np.asarray(sizes)[tid]).astype(np.int64)
        tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
        e_roots = np.stack([tree(_tag(arity), flat[int(off[t]):int(off[t + 1])])[0] for t in range(len(sizes))])
        jobs.append((arity, sizes, d, d_off, roots, d_lv, tid, lid, e_roots[tid]))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for rep in range(20):
        outs = []
        for (arity, sizes, d, d_off, roots, d_lv, tid, lid, _), s in zip(jobs, streams):
            with torch.cuda.stream(s):
                o = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid)
                outs.append((o, _verify(gpu_ctx, arity, o, roots, len(sizes))))
        torch.cuda.synchronize()
        for (arity, sizes, d, d_off, roots, d_lv, tid, lid, exp), (o, ok) in zip(jobs, outs):
            assert np.array_equal(_np(o["back"]), exp), (rep, arity)
            assert int(ok.sum()) == len(tid), (rep, arity)


@pytest.mark.parametrize("arity", [4, 2])
def test_graph_capture_of_openings_and_verify_replays_on_new_leaf_ids(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 5, 17, 256, 1000, 3, 64] * 20
    off = TS.offsets(sizes)
    d, d_off = _torch(oracle_mod.fill_random(0x61 + arity, int(off[-1]))), _torch(off)
    n_trees, max_leaves, k = len(sizes), 1000, 5000
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, n_trees, max_leaves)
    rng = np.random.default_rng(arity)

    def draw():
        tid = rng.integers(0, n_trees, k)
        return tid, (rng.random(k) * np.asarray(sizes)[tid]).astype(np.int64)
    tid, lid = draw()
    d_tid, d_lid = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64))
    D = TS.depth(max_leaves, arity)
    out = (torch.empty((k, 4), dtype=torch.int64, device=d.device), torch.empty((k, D, arity - 1, 4), dtype=torch.int64, device=d.device),
           torch.empty((k, D), dtype=torch.uint8, device=d.device), torch.empty((k,), dtype=torch.uint8, device=d.device))
    ok = torch.zeros(k, dtype=torch.uint8, device=d.device)
    tag = _tag(arity)

    def both():
        gpu_ctx.merkle_forest_ragged_openings_device(d, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, k, out=out, arity=arity)
        gpu_ctx.merkle_forest_ragged_verify_device(tag, out[0], out[1], out[2], out[3], D, d_tid, roots, n_trees, ok, k, arity=arity)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        both()  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    assert int(ok.sum()) == k
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        both()
    tid2, lid2 = draw()
    tid2[0], lid2[0] = n_trees, 0  # one bad opening among the new ones
    d_tid.copy_(_torch(tid2.astype(np.uint32)))
    d_lid.copy_(_torch(lid2.astype(np.uint64)))
    ok.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _np(ok).tolist() == [0] + [1] * (k - 1)
    assert np.array_equal(_np(out[0])[1:], _np(d)[off[tid2[1:]].astype(np.int64) + lid2[1:]])
    assert int(out[3][0]) == BAD


@pytest.mark.parametrize("arity", [4, 2])
def test_leaf_buffer_past_4_gib(gpu_ctx, oracle_mod, arity):
    import torch
    start = (1 << 27) + 3  # more than 2^27 leaves (4 GiB) before the first tree
    sizes = [1, 9, 1000, 64, 4097]
    off = TS.offsets(sizes, start=start)
    n_leaves = int(off[-1]) + 5
    need = n_leaves * 32 + TS.levels_bound(n_leaves, len(sizes), 4097, arity) * 32 + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d GiB of free HBM" % (need >> 30))
    d = torch.zeros((n_leaves, 4), dtype=torch.int64, device="cuda:0")
    tail = oracle_mod.fill_random(0x64 + arity, int(off[-1]) - start)
    d[start:int(off[-1])] = _torch(tail)
    d_off = _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), 4097)
    t = len(sizes) - 1
    lid = np.array([0, 1, 4095, 4096, 2048, 777])
    o = _open(gpu_ctx, arity, d, d_off, len(sizes), 4097, d_lv, np.full(lid.size, t), lid)
    ok = _verify(gpu_ctx, arity, o, roots, len(sizes))
    torch.cuda.synchronize()
    last = tail[-4097:]
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    r, lv, _ = tree(_tag(arity), last, want_levels=True)
    from poseidon252_amd import merkle as M
    s, p = M.merkle4_openings(last, lv, lid) if arity == 4 else _merkle2_openings(last, lv, lid)
    assert np.array_equal(_np(o["leaves"]), last[lid])
    assert np.array_equal(_np(o["sib"]), s.reshape(lid.size, -1, arity - 1, 4)) and np.array_equal(_np(o["pos"]), p)
    assert np.array_equal(_np(o["back"]), np.tile(r, (lid.size, 1))) and int(ok.sum()) == lid.size
    del d, d_lv, o
    torch.cuda.empty_cache()


def test_trim_gives_the_scratch_back(oracle_mod):
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    try:
        arity, sizes = 4, [4 ** 5] * 64
        off = TS.offsets(sizes)
        d, d_off = _torch(oracle_mod.fill_random(0x77, int(off[-1]))), _torch(off)
        roots, d_lv = _build(ctx, arity, d, d_off, len(sizes), max(sizes))
        k = 1 << 21
        rng = np.random.default_rng(3)
        tid, lid = rng.integers(0, len(sizes), k), rng.integers(0, 4 ** 5, k)
        d_tid, d_lid = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64))
        D = 5
        out = (torch.empty((k, 4), dtype=torch.int64, device=d.device), torch.empty((k, D, 3, 4), dtype=torch.int64, device=d.device),
               torch.empty((k, D), dtype=torch.uint8, device=d.device), torch.empty((k,), dtype=torch.uint8, device=d.device))
        ok = torch.zeros(k, dtype=torch.uint8, device=d.device)
        torch.cuda.synchronize()
        ctx.trim()
        free0 = torch.cuda.mem_get_info()[0]
        ctx.merkle_forest_ragged_openings_device(d, d_off, len(sizes), max(sizes), d_lv, d_tid, d_lid, k, out=out, arity=arity)
        ctx.merkle_forest_ragged_verify_device(_tag(arity), out[0], out[1], out[2], out[3], D, d_tid, roots, len(sizes), ok, k, arity=arity)
        torch.cuda.synchronize()
        assert int(ok.sum()) == k
        held = free0 - torch.cuda.mem_get_info()[0]
        assert held >= k * 40 - (64 << 20), "the calls did not use context-owned scratch? held %d" % held  # roots + order: 80 MiB
        ctx.trim()
        free1 = torch.cuda.mem_get_info()[0]
        assert abs(free0 - free1) <= 64 << 20, "p252_trim left %d bytes allocated" % (free0 - free1)
        assert ctx.scratch_residue() == 0
    finally:
        ctx.close()


# V1 floor: 0.9 x the ratio measured on an MI355X (profiles/forest_openings.txt: 1.004 for arity 4, 0.997 for arity 2), rounded down
# to two digits — the margin is for box-to-box clock spread, which a same-process ratio mostly cancels
V1_FLOOR = {4: 0.90, 2: 0.89}

_V2_CHILD = r"""
import sys, json, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import poseidon252_amd as P
from helpers import forest as T
print(json.dumps(T._v2_rate(P.Context(0))))
"""


@pytest.mark.parametrize("arity,per", [(4, 4 ** 6), (2, 2 ** 12)])
def test_v1_equal_depths_keep_the_fixed_depth_rate(gpu_ctx, arity, per):
    """V1 of profiles/forest_openings.txt at a quarter of its size: path_ragged against p252_merkle{4,2}_path_batch_device on the same
    openings, alternated in one process"""
    import torch
    n_trees, k = 1024, 1 << 18
    d = torch.randint(0, 1 << 60, (n_trees * per, 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(TS.offsets([per] * n_trees))
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, n_trees, per)
    rng = np.random.default_rng(1)
    o = _open(gpu_ctx, arity, d, d_off, n_trees, per, d_lv, rng.integers(0, n_trees, k), rng.integers(0, per, k))
    D = o["D"]
    exp = torch.empty_like(o["back"])
    fixed_fn = gpu_ctx.merkle4_path_batch_device if arity == 4 else gpu_ctx.merkle2_path_batch_device
    fixed = lambda: fixed_fn(_tag(arity), o["leaves"], o["sib"], o["pos"], D, exp, k)  # noqa: E731
    ragged = lambda: gpu_ctx.merkle_path_ragged_device(_tag(arity), o["leaves"], o["sib"], o["pos"], o["dep"], D, o["back"], k, arity=arity)  # noqa: E731
    fixed(), ragged()
    tf, tr = [], []
    for _ in range(9):
        tf.append(_median_ms(fixed, 1))
        tr.append(_median_ms(ragged, 1))
    assert torch.equal(exp, o["back"])
    ratio = float(np.median(tf)) / float(np.median(tr))
    print("V1 arity %d: fixed %.3f ms, ragged %.3f ms, ratio %.3f" % (arity, np.median(tf), np.median(tr), ratio))
    assert ratio >= V1_FLOOR[arity], "ragged %.3f ms vs fixed depth %.3f ms: ratio %.3f" % (np.median(tr), np.median(tf), ratio)
    if os.environ.get("P252_PERF_STRICT") == "1":  # the projection itself, without the margin
        assert ratio >= 0.90, ratio


def test_v2_sorted_is_not_slower_than_unsorted(gpu_ctx):
    """(a sanity check: the sort must pay for itself on mixed depths; the identity order needs a fresh process, the switch is read once)"""
    import json
    sorted_rate = _v2_rate(gpu_ctx)
    code = _V2_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, P252_RAGGED_SORT="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    unsorted_rate = json.loads(r.stdout.strip().splitlines()[-1])
    print("V2: sorted %.3e levels/s, unsorted %.3e levels/s" % (sorted_rate["levels_per_s"], unsorted_rate["levels_per_s"]))
    assert sorted_rate["levels_per_s"] >= 0.98 * unsorted_rate["levels_per_s"], (sorted_rate, unsorted_rate)


def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_openings_api", tmp_path))
