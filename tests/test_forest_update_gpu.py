"""Leaf updates anywhere in a forest of trees of different sizes in one call (p252_merkle{4,2}_forest_ragged_update_device;
csrc/forest_update.hip) on the GPU: leaves, levels and roots against a fresh build of the modified leaves and against the oracle,
the number of digests against the numpy count of distinct dirty nodes, bad updates, edge sizes, both digest kernels, the openings
of the changed leaves, streams, graph capture, p252_trim, a leaf buffer past 4 GiB, the C++ mirror and the speed floor."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.forest import (SENTINEL, _build, _check_against_fresh_build, _distinct_pairs, _forest, _median_ms, _mix, _np, _open, _tag, _torch,
                            _tree, _update, _verify, dirty_count)
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _used(sizes, arity):
    from poseidon252_amd import levels_len
    return sum(levels_len(int(n), arity) for n in sizes if n > 0)


# ---- 1. parity ----
@pytest.mark.parametrize("arity", [4, 2])
def test_parity_with_a_fresh_build_and_the_oracle(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = _mix(arity) * 2
    np.random.default_rng(arity).shuffle(sizes)
    off = TS.offsets(sizes, start=5)  # offsets[0] != 0
    flat = oracle_mod.fill_random(0x0AD0 + arity, int(off[-1]) + 3)
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
    torch.cuda.synchronize()
    before_lv, used = d_lv.clone(), _used(sizes, arity)
    assert bool((d_lv[used:] == SENTINEL).all()) and not bool((d_lv[:used] == SENTINEL).all(dim=1).any())
    rng = np.random.default_rng(31 + arity)
    untouched = [0, 5, len(sizes) - 1, int(np.argmax(sizes))]
    trees = [t for t in range(len(sizes)) if t not in untouched]
    tid, lid = _distinct_pairs(sizes, rng, 500, trees)
    new = oracle_mod.fill_random(0x0AE0 + arity, tid.size)
    d_roots = torch.full((len(sizes), 4), SENTINEL, dtype=torch.int64, device=d.device)
    bad, hashed = _update(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    assert int(bad) == 0 and int(hashed) == dirty_count(sizes, tid, lid, arity)
    _check_against_fresh_build(gpu_ctx, oracle_mod, arity, flat, off, tid, lid, new, d, d_lv, d_roots)
    # the blocks of the untouched trees, and everything past the used length
    from poseidon252_amd import levels_len
    lo = np.concatenate([[0], np.cumsum([levels_len(n, arity) for n in sizes])]).astype(np.int64)
    for t in untouched:
        assert torch.equal(d_lv[lo[t]:lo[t + 1]], before_lv[lo[t]:lo[t + 1]]), t
    assert torch.equal(d_lv[used:], before_lv[used:])
    assert not torch.equal(d_lv[:used], before_lv[:used])


# ---- 2. each dirty node once ----
@pytest.mark.parametrize("arity", [4, 2])
def test_each_dirty_node_is_hashed_once(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = _mix(arity) * 3
    off = TS.offsets(sizes, start=2)
    flat = oracle_mod.fill_random(0x0B00 + arity, int(off[-1]))
    rng = np.random.default_rng(7 + arity)
    big = int(np.argmax(sizes))
    node = 5  # all children of node 5 of level 1 of the largest tree: one dirty node per level
    cases = {"sparse": _distinct_pairs(sizes, rng, 40),
             "every leaf": _distinct_pairs(sizes, rng, int(sum(sizes))),
             "one node": (np.full(arity, big), node * arity + np.arange(arity))}
    for name, (tid, lid) in cases.items():
        d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
        new = oracle_mod.fill_random(0x0B10 + arity, len(tid))
        d_roots = torch.full((len(sizes), 4), SENTINEL, dtype=torch.int64, device=d.device)
        bad, hashed = _update(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, new, d_roots)
        torch.cuda.synchronize()
        want = dirty_count(sizes, tid, lid, arity)
        assert int(bad) == 0 and int(hashed) == want, (name, int(hashed), want)
        if name == "every leaf":
            assert want == _used(sizes, arity)
        if name == "one node":
            assert want == TS.depth(sizes[big], arity)
        _check_against_fresh_build(gpu_ctx, oracle_mod, arity, flat, off, tid, lid, new, d, d_lv, d_roots)


# ---- 3. bad updates, duplicates ----
@pytest.mark.parametrize("arity", [4, 2])
def test_bad_updates_are_counted_and_write_nothing(gpu_ctx, oracle_mod, arity):
    """(every bad input here is one the kernels are specified to bound-check)"""
    import torch
    flat = oracle_mod.fill_random(0x0BAD + arity, 1000)
    # max_leaves 300: t1 empty, t3 longer than max_leaves, t5 behind decreasing offsets, t9 past n_leaves; t6 overlaps t4 and is good
    off = np.array([0, 10, 10, 30, 340, 370, 360, 365, 600, 800, 1010], dtype=np.uint64)
    n_trees, max_leaves = 10, 300
    g_tid = [0, 2, 7, 7, 7, 7, 8, 8, 0, 2]
    g_lid = [9, 0, 5, 100, 234, 77, 199, 5, 0, 19]  # (tree 7's leaves 0 .. 4 are tree 4's last five as well: left alone)
    b_tid = [10, 0x7fffffff, 0, 1, 3, 5, 9, 7, 8]
    b_lid = [0, 0, 10, 0, 0, 0, 0, 1 << 40, 200]  # (leaf id = n_t for trees 0 and 8, 2^40 for tree 7)
    order = np.random.default_rng(arity).permutation(len(g_tid) + len(b_tid))
    tid, lid = np.array(g_tid + b_tid)[order], np.array(g_lid + b_lid)[order]
    is_good = (order < len(g_tid))
    new = oracle_mod.fill_random(0x0BB0 + arity, tid.size)
    sizes = [10, 0, 20, 0, 30, 0, 5, 235, 200, 0]  # what the build takes the trees for (0: a bad tree)
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off, max_leaves)
    d_roots = torch.full((n_trees, 4), SENTINEL, dtype=torch.int64, device=d.device)
    bad, hashed = _update(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    assert int(bad) == len(b_tid)
    assert int(hashed) == dirty_count(sizes, tid[is_good], lid[is_good], arity)
    want = flat.copy()
    want[off[tid[is_good]].astype(np.int64) + lid[is_good]] = new[is_good]
    assert np.array_equal(_np(d), want)  # the valid neighbours applied, nothing written for the bad ones
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off, max_leaves)
    torch.cuda.synchronize()
    assert torch.equal(d_lv, f_lv)
    touched = sorted(set(g_tid))
    assert torch.equal(d_roots[touched], f_roots[touched])
    rest = [t for t in range(n_trees) if t not in touched]
    assert bool((d_roots[rest] == SENTINEL).all())
    tree = _tree(oracle_mod, arity)
    for t in touched:
        assert np.array_equal(_np(d_roots)[t], tree(_tag(arity), want[int(off[t]):int(off[t + 1])])[0]), t
    # the same list with every update repeated (the same value): the same bytes, the same number of digests
    first = int(hashed)
    bad2, hashed2 = _update(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, np.tile(tid, 2), np.tile(lid, 2), np.tile(new, (2, 1)), d_roots)
    torch.cuda.synchronize()
    assert int(bad2) == 2 * len(b_tid) and int(hashed2) == first
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(d_roots[touched], f_roots[touched])


# ---- 4. edges ----
@pytest.mark.parametrize("arity", [4, 2])
def test_edge_sizes(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import _lib
    # D == 0: every tree a single leaf, no levels at all; the roots follow the leaves
    n_trees = 50
    flat = oracle_mod.fill_random(0x0D0 + arity, n_trees)
    d, d_off = _torch(flat), _torch(TS.offsets([1] * n_trees))
    d_roots = torch.full((n_trees, 4), SENTINEL, dtype=torch.int64, device=d.device)
    tid, lid = np.array([3, 49, 0, 50, 3 + 8]), np.array([0, 0, 0, 0, 1])
    new = oracle_mod.fill_random(0x0D1 + arity, tid.size)
    bad, hashed = _update(gpu_ctx, arity, d, d_off, n_trees, 1, None, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    assert int(bad) == 2 and int(hashed) == 0
    want = flat.copy()
    want[[3, 49, 0]] = new[:3]
    assert np.array_equal(_np(d), want)
    assert np.array_equal(_np(d_roots)[[3, 49, 0]], new[:3])
    assert int((d_roots == SENTINEL).all(dim=1).sum()) == n_trees - 3
    # k == 0: nothing enqueued, the C call takes NULL buffers
    L = _lib.lib()
    fn = L.p252_merkle4_forest_ragged_update_device if arity == 4 else L.p252_merkle2_forest_ragged_update_device
    assert fn(gpu_ctx._h, None, None, 0, None, 0, 0, None, None, None, None, 0, None, None, None, None) == 0
    # one tree of one leaf
    one = oracle_mod.fill_random(0x0D2 + arity, 1)
    d1, d1_off = _torch(one), _torch(TS.offsets([1]))
    r1 = torch.full((1, 4), SENTINEL, dtype=torch.int64, device=d.device)
    bad, hashed = _update(gpu_ctx, arity, d1, d1_off, 1, 1, None, [0], [0], new[:1], r1)
    torch.cuda.synchronize()
    assert int(bad) == 0 and int(hashed) == 0 and np.array_equal(_np(d1), new[:1]) and np.array_equal(_np(r1), new[:1])


def test_one_tree_arity_2_against_the_oracle_with_levels(gpu_ctx, oracle_mod):
    import torch
    n = 1000
    flat, off = oracle_mod.fill_random(0x0D20, n), TS.offsets([n])
    d, d_off, roots, d_lv = _forest(gpu_ctx, 2, flat, off, tail=0)
    rng = np.random.default_rng(2)
    lid = rng.choice(n, 120, replace=False)
    new = oracle_mod.fill_random(0x0D21, lid.size)
    bad, hashed = _update(gpu_ctx, 2, d, d_off, 1, n, d_lv, np.zeros(lid.size, np.int64), lid, new, roots)
    torch.cuda.synchronize()
    want = flat.copy()
    want[lid] = new
    r, lv, _ = oracle_mod.merkle2_tree(_tag(2), want, want_levels=True)
    assert int(bad) == 0 and int(hashed) == dirty_count([n], np.zeros(lid.size, np.int64), lid, 2)
    assert np.array_equal(_np(roots)[0], r) and np.array_equal(_np(d_lv)[:lv.shape[0]], lv) and np.array_equal(_np(d), want)


def test_one_tree_arity_4_against_the_single_tree_update(gpu_ctx, oracle_mod):
    import torch
    n = 4 ** 6 + 77
    flat, off = oracle_mod.fill_random(0x0D40, n), TS.offsets([n])
    d, d_off, roots, d_lv = _forest(gpu_ctx, 4, flat, off, tail=0)
    d_b, lv_b = d.clone(), d_lv.clone()
    rng = np.random.default_rng(4)
    lid = rng.choice(n, 900, replace=False)
    new = oracle_mod.fill_random(0x0D41, lid.size)
    _update(gpu_ctx, 4, d, d_off, 1, n, d_lv, np.zeros(lid.size, np.int64), lid, new, roots)
    root_b = torch.zeros((1, 4), dtype=torch.int64, device=d.device)
    gpu_ctx.merkle4_update_device(_tag(4), d_b, n, lv_b, _torch(lid.astype(np.uint32)), _torch(new), lid.size, d_root=root_b)
    torch.cuda.synchronize()
    assert torch.equal(d, d_b) and torch.equal(d_lv, lv_b) and torch.equal(roots, root_b)


# ---- 5. both digest kernels ----
def _wide(arity, oracle_mod):
    sizes = [(4 ** 8 if arity == 4 else 2 ** 16)] * 4 + _mix(arity)
    off = TS.offsets(sizes, start=1)
    return sizes, off, oracle_mod.fill_random(0x0E00 + arity, int(off[-1]))


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import poseidon252_amd as P
from helpers import forest as T
z = np.load(%(inp)r)
arity = int(z["arity"])
ctx = P.Context(0)
d, d_off, roots, d_lv = T._forest(ctx, arity, z["flat"], z["off"])
bad, hashed = T._update(ctx, arity, d, d_off, len(z["off"]) - 1, int(z["max_leaves"]), d_lv, z["tid"], z["lid"], z["new"], roots)
torch.cuda.synchronize()
np.savez(%(out)r, leaves=T._np(d), levels=T._np(d_lv), roots=T._np(roots), hashed=int(hashed), bad=int(bad))
"""


@pytest.mark.parametrize("arity", [4, 2])
def test_both_digest_kernels_give_the_same_bytes(gpu_ctx, oracle_mod, tmp_path, arity):
    import torch
    sizes, off, flat = _wide(arity, oracle_mod)
    rng = np.random.default_rng(50 + arity)
    small = None
    for k in (100, 45000):  # the lane groups on every level; the one-lane kernel on the wide levels
        tid, lid = _distinct_pairs(sizes, rng, k)
        new = oracle_mod.fill_random(0x0E10 + arity + k, k)
        d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
        bad, hashed = _update(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, new, roots)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(hashed) == dirty_count(sizes, tid, lid, arity), k
        want = flat.copy()
        want[off[tid].astype(np.int64) + lid] = new
        _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
        torch.cuda.synchronize()
        assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots), k
        if k == 100:
            small = (tid, lid, new, _np(d), _np(d_lv), _np(roots), int(hashed))
    # the small case again without the lane-group kernels (the switch is read once per process)
    tid, lid, new, e_leaves, e_levels, e_roots, e_hashed = small
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, arity=arity, flat=flat, off=off, max_leaves=max(sizes), tid=tid, lid=lid, new=new)
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), inp=inp, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, P252_COOP_MAX_NODES="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["leaves"], e_leaves) and np.array_equal(z["levels"], e_levels) and np.array_equal(z["roots"], e_roots)
    assert int(z["hashed"]) == e_hashed and int(z["bad"]) == 0


# ---- 6. end to end ----
@pytest.mark.parametrize("arity", [4, 2])
def test_openings_of_the_changed_leaves_verify_against_the_new_roots_only(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = _mix(arity) * 2
    off = TS.offsets(sizes, start=4)
    flat = oracle_mod.fill_random(0x0F00 + arity, int(off[-1]))
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
    old_roots = roots.clone()
    rng = np.random.default_rng(arity)
    tid, lid = _distinct_pairs(sizes, rng, 300)
    every = np.arange(len(sizes))  # and a leaf of every tree: every old root is stale
    pairs = np.unique(np.stack([np.concatenate([tid, every]), np.concatenate([lid, (rng.random(every.size) * np.asarray(sizes)).astype(np.int64)])], axis=1), axis=0)
    tid, lid = pairs[:, 0], pairs[:, 1]
    new = oracle_mod.fill_random(0x0F10 + arity, tid.size)
    _update(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, new, roots)
    o = _open(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid)
    ok_new = _verify(gpu_ctx, arity, o, roots, len(sizes))
    ok_old = _verify(gpu_ctx, arity, o, old_roots, len(sizes))
    torch.cuda.synchronize()
    assert np.array_equal(_np(o["leaves"]), new)
    assert _np(ok_new).tolist() == [1] * tid.size and _np(ok_old).tolist() == [0] * tid.size


# ---- 7. streams, capture, trim ----
def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for j, (arity, sizes) in enumerate(((4, [3000, 7, 900, 1] * 10), (2, [65, 1024, 2, 300] * 10))):
        off = TS.offsets(sizes)
        flat = oracle_mod.fill_random(0x5F0 + j, int(off[-1]))
        d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
        tid, lid = _distinct_pairs(sizes, np.random.default_rng(j), 12000)
        news = [oracle_mod.fill_random(0x600 + 16 * j + r, tid.size) for r in range(2)]
        exp = []
        for new in news:
            want = flat.copy()
            want[off[tid].astype(np.int64) + lid] = new
            _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
            exp.append((f_roots, f_lv))
        jobs.append(dict(arity=arity, n=len(sizes), m=max(sizes), d=d, d_off=d_off, roots=roots, d_lv=d_lv, tid=_torch(tid.astype(np.uint32)),
                         lid=_torch(lid.astype(np.uint64)), news=[_torch(x) for x in news], exp=exp, k=tid.size, dirty=dirty_count(sizes, tid, lid, arity),
                         hashed=torch.zeros(1, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for rep in range(10):
        for J, s in zip(jobs, streams):
            with torch.cuda.stream(s):
                J["hashed"].zero_()
                gpu_ctx.merkle_forest_ragged_update_device(_tag(J["arity"]), J["d"], J["d_off"], J["n"], J["m"], J["d_lv"], J["tid"], J["lid"],
                                                           J["news"][rep & 1], J["k"], d_roots=J["roots"], d_n_hashed=J["hashed"], arity=J["arity"])
        torch.cuda.synchronize()
        for J in jobs:
            f_roots, f_lv = J["exp"][rep & 1]
            assert torch.equal(J["d_lv"], f_lv) and torch.equal(J["roots"], f_roots), (rep, J["arity"])
            assert int(J["hashed"]) == J["dirty"], (rep, J["arity"])


@pytest.mark.parametrize("arity", [4, 2])
def test_graph_capture_replays_on_new_values(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 5, 17, 256, 1000, 3, 64] * 20
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0x0610 + arity, int(off[-1]))
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
    n_trees, max_leaves, k = len(sizes), 1000, 5000
    tid, lid = _distinct_pairs(sizes, np.random.default_rng(arity), k)
    tid[0], lid[0] = n_trees, 0  # one bad update in the list
    d_tid, d_lid = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64))
    d_new = _torch(oracle_mod.fill_random(0x0620 + arity, k))
    bad = torch.zeros(1, dtype=torch.int32, device=d.device)
    hashed = torch.zeros(1, dtype=torch.int64, device=d.device)
    tag = _tag(arity)

    def call():
        gpu_ctx.merkle_forest_ragged_update_device(tag, d, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, d_new, k, d_roots=roots, d_n_bad=bad,
                                                   d_n_hashed=hashed, arity=arity)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    new2 = oracle_mod.fill_random(0x0630 + arity, k)
    d_new.copy_(_torch(new2))
    bad.zero_()
    hashed.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = flat.copy()
    want[off[tid[1:]].astype(np.int64) + lid[1:]] = new2[1:]
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
    torch.cuda.synchronize()
    assert int(bad) == 1 and int(hashed) == dirty_count(sizes, tid[1:], lid[1:], arity)
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots)


def test_trim_gives_the_scratch_back(oracle_mod):
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    try:
        arity, sizes = 4, [4 ** 5] * 2048
        off = TS.offsets(sizes)
        d = torch.randint(0, 1 << 60, (int(off[-1]), 4), dtype=torch.int64, device="cuda:0")
        d_off = _torch(off)
        roots, d_lv = _build(ctx, arity, d, d_off, len(sizes), max(sizes))
        k = 1 << 21
        lid_all = np.arange(k, dtype=np.int64)  # every leaf of the forest
        d_tid, d_lid = _torch((lid_all >> 10).astype(np.uint32)), _torch((lid_all & 1023).astype(np.uint64))
        d_new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device="cuda:0")
        hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.trim()
        free0 = torch.cuda.mem_get_info()[0]

        def call():
            ctx.merkle_forest_ragged_update_device(_tag(arity), d, d_off, len(sizes), max(sizes), d_lv, d_tid, d_lid, d_new, k, d_roots=roots,
                                                   d_n_hashed=hashed, arity=arity)
        call()
        torch.cuda.synchronize()
        assert int(hashed) == _used(sizes, arity)
        held = free0 - torch.cuda.mem_get_info()[0]
        # the two lists (32 bytes per update) and the claim table (2^22 slots of 8 bytes): 96 MiB
        assert held >= k * 48 - (64 << 20), "the call did not use context-owned scratch? held %d" % held
        assert held <= k * 64 + (64 << 20), "more than 64 bytes of scratch per update: held %d" % held
        ctx.trim()
        free1 = torch.cuda.mem_get_info()[0]
        assert abs(free0 - free1) <= 64 << 20, "p252_trim left %d bytes allocated" % (free0 - free1)
        assert ctx.scratch_residue() == 0
        hashed.zero_()
        call()  # the next call takes the scratch again
        fresh_roots, fresh_lv = _build(ctx, arity, d, d_off, len(sizes), max(sizes))
        torch.cuda.synchronize()
        assert int(hashed) == _used(sizes, arity) and torch.equal(roots, fresh_roots) and torch.equal(d_lv, fresh_lv)
    finally:
        ctx.close()


# ---- 8. 64-bit indexing ----
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
    tail = oracle_mod.fill_random(0x0640 + arity, int(off[-1]) - start)
    d[start:int(off[-1])] = _torch(tail)
    d_off = _torch(off)
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, len(sizes), 4097)
    t = len(sizes) - 1
    lid = np.array([0, 1, 4095, 4096, 2048, 777])
    new = oracle_mod.fill_random(0x0650 + arity, lid.size)
    bad, hashed = _update(gpu_ctx, arity, d, d_off, len(sizes), 4097, d_lv, np.full(lid.size, t), lid, new, roots)
    torch.cuda.synchronize()
    last = tail[-4097:].copy()
    last[lid] = new
    r, lv, _ = _tree(oracle_mod, arity)(_tag(arity), last, want_levels=True)
    assert int(bad) == 0 and int(hashed) == dirty_count([4097], np.zeros(lid.size, np.int64), lid, arity)
    assert np.array_equal(_np(d[int(off[t]):int(off[t + 1])]), last) and np.array_equal(_np(roots)[t], r)
    used = _used(sizes, arity)
    assert np.array_equal(_np(d_lv[used - lv.shape[0]:used]), lv)
    assert not bool(d[:start].any())  # nothing landed at the indices' low 32 bits
    del d, d_lv
    torch.cuda.empty_cache()


# ---- 9. the C++ mirror ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_update_api", tmp_path))


# ---- 10. the speed floor ----
# U1 floor: 0.9 x the ratio measured on an MI355X for this size (profiles/forest_update.txt, "U1 4^11 leaves, k = 2^18": 2.590), rounded
# down to two digits — the margin is for box-to-box clock spread, which a same-process alternated ratio mostly cancels.  Never
# below 1.0: de-duplication that does not pay for its claim passes is not done.
U1_FLOOR = 2.33


def test_u1_hashing_each_dirty_node_once_beats_k_digests_per_level(gpu_ctx):
    """U1 of profiles/forest_update.txt on a 4^11-leaf tree, k = 2^18 distinct random leaves: the forest call (a forest of one tree)
    against p252_merkle4_update_device on the same updates, alternated in one process"""
    import torch
    n, k = 4 ** 11, 1 << 18
    d = torch.randint(0, 1 << 60, (n, 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(TS.offsets([n]))
    roots, d_lv = _build(gpu_ctx, 4, d, d_off, 1, n)
    lid = np.random.default_rng(1).choice(n, k, replace=False)
    d_tid, d_lid, d_idx = _torch(np.zeros(k, np.uint32)), _torch(lid.astype(np.uint64)), _torch(lid.astype(np.uint32))
    d_new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device="cuda:0")
    d_b, lv_b, root_b = d.clone(), d_lv.clone(), torch.zeros((1, 4), dtype=torch.int64, device="cuda:0")
    tag = _tag(4)
    new = lambda: gpu_ctx.merkle_forest_ragged_update_device(tag, d, d_off, 1, n, d_lv, d_tid, d_lid, d_new, k, d_roots=roots)  # noqa: E731
    old = lambda: gpu_ctx.merkle4_update_device(tag, d_b, n, lv_b, d_idx, d_new, k, d_root=root_b)  # noqa: E731
    new(), old()
    t_new, t_old = [], []
    for _ in range(9):
        t_old.append(_median_ms(old, 1))
        t_new.append(_median_ms(new, 1))
    assert torch.equal(d, d_b) and torch.equal(d_lv, lv_b) and torch.equal(roots, root_b)
    ratio = float(np.median(t_old)) / float(np.median(t_new))
    print("U1 4^11 leaves, k = 2^18: per-level k digests %.3f ms, each dirty node once %.3f ms, ratio %.3f" % (np.median(t_old), np.median(t_new), ratio))
    assert ratio >= U1_FLOOR, "forest update %.3f ms vs merkle4_update %.3f ms: ratio %.3f" % (np.median(t_new), np.median(t_old), ratio)
