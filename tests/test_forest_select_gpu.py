"""Trees of built forests gathered into a new forest (p252_merkle{4,2}_forest_ragged_select_device_into; the select of
csrc/forest_ragged.hip) on the GPU.  The expected outputs are the sources' own arrays, gathered in numpy as the model of
tests/forestselect.py lays them out, and a fresh merkle_forest_ragged_device build of the gathered leaves — never the select itself:
offsets, leaves, the used levels, roots and the bad count, with a sentinel tail behind every output; tile edges; refused picks and the
cap rule; more picks than one trip of the scan; offsets past 4 GiB; the result under the other forest calls; two streams, graph
capture, the host refusals through ctypes, the C++ mirror and the bench tool."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import forestselect as FS
from helpers.forest import SENTINEL, Grown, _append, _build, _forest, _mix, _np, _open, _outputs, _tag, _torch, _tree, _update, _verify
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ARITIES = [4, 2]
TAIL = 7
U64_MAX = 2 ** 64 - 1


class Src:
    """a source forest on the device, with what numpy needs of it on the host"""

    def __init__(self, ctx, oracle_mod, arity, sizes, seed, max_leaves=None, bad=()):
        sizes = [int(s) for s in sizes]
        self.arity, self.sizes, self.bad, self.n_trees = arity, sizes, set(bad) | {t for t, s in enumerate(sizes) if s == 0}, len(sizes)
        self.max_leaves = max_leaves or max(sizes)
        self.flat, self.off = oracle_mod.fill_random(seed, sum(sizes)), TS.offsets(sizes)
        self.d, self.d_off, self.roots, self.d_lv = _forest(ctx, arity, self.flat, self.off, self.max_leaves)
        self.lo = FS.level_starts_of(sizes, self.bad, arity)

    def view(self):
        return (self.d, self.d_off, self.n_trees, self.max_leaves, self.d_lv, self.roots)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.flat, self.off, self.lo, _np(self.d_lv), _np(self.roots)


def _buffers(arity, cap, n_pick, max_leaves):
    """sentinel-filled outputs with TAIL elements past what the call may use, and the zeroed bad count"""
    import torch
    out = _outputs(arity, cap, n_pick, max_leaves, tail=TAIL)
    return out, torch.zeros(1, dtype=torch.int32, device="cuda:0")


def _method(ctx, arity):
    return ctx.merkle4_forest_ragged_select_device if arity == 4 else ctx.merkle2_forest_ragged_select_device


def _select(ctx, arity, A, B, d_pick, n_pick, cap, out, bad):
    max_leaves = max(A.max_leaves, B.max_leaves if B is not None else 0)
    bound = TS.levels_bound(cap, n_pick, max_leaves, arity)
    _method(ctx, arity)(A.view(), B.view() if B is not None else None, d_pick, n_pick, out[0][:cap], out[1][:n_pick + 1],
                        out[2][:bound] if bound else None, out[3][:n_pick], bad)


def _run(ctx, arity, A, B, pick, cap):
    """select, compare with the model and the numpy gather, sentinel tails included -> (model, outputs)"""
    import torch
    pick = [int(p) for p in pick]
    M = FS.select_model(arity, A.sizes, A.bad, B.sizes if B is not None else [], B.bad if B is not None else [], pick, cap)
    out, bad = _buffers(arity, cap, len(pick), max(A.max_leaves, B.max_leaves if B is not None else 0))
    _select(ctx, arity, A, B, _torch(np.asarray(pick, np.uint64)), len(pick), cap, out, bad)
    torch.cuda.synchronize()
    leaves, levels, roots = FS.gather(M, arity, A.host(), B.host() if B is not None else None)
    sent = np.uint64(SENTINEL & U64_MAX)
    got_leaves, got_off, got_lv, got_roots = (_np(t) for t in out)
    n, used, lused = len(pick), leaves.shape[0], levels.shape[0]
    assert used == int(M["offsets_new"][-1]) and lused == int(M["level_starts"][-1])
    assert np.array_equal(got_off[:n + 1], M["offsets_new"]) and (got_off[n + 1:] == sent).all()
    assert np.array_equal(got_leaves[:used], leaves) and (got_leaves[used:] == sent).all()
    assert np.array_equal(got_lv[:lused], levels) and (got_lv[lused:] == sent).all()
    assert np.array_equal(got_roots[:n], roots) and (got_roots[n:] == sent).all()
    assert int(bad) == M["n_bad"], (int(bad), M["n_bad"])
    for j in np.flatnonzero(M["refused"]):
        assert not got_roots[j].any() and got_off[j] == got_off[j + 1], j
    return M, out


def _fresh_like(ctx, arity, out, n_pick, cap, max_leaves):
    """a fresh build of the select's leaves and offsets into sentinel-filled buffers of the same sizes -> (levels, roots, n_bad)"""
    import torch
    levels, roots = torch.full_like(out[2], SENTINEL), torch.full_like(out[3], SENTINEL)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    bound = TS.levels_bound(cap, n_pick, max_leaves, arity)
    ctx.merkle_forest_ragged_device(_tag(arity), out[0][:cap], out[1][:n_pick + 1], n_pick, max_leaves, roots[:n_pick], levels[:bound], bad, arity=arity)
    torch.cuda.synchronize()
    return levels, roots, bad


def _sizes_b(arity):
    a = arity
    return [7, 1, 33, 129, 2, 100, a ** 3 + 1, 5, a ** 4, 1, 11, 2 * a, 31, 64, 6, 1, a ** 5 - 1, 9, 250, 3, 12]


def _mixed_case(ctx, oracle_mod, arity):
    A = Src(ctx, oracle_mod, arity, _mix(arity) + [1] * 5, 0x5E10 + arity)
    B = Src(ctx, oracle_mod, arity, _sizes_b(arity), 0x5E20 + arity)
    rng = np.random.default_rng(0x5E + arity)
    ids = list(range(A.n_trees + B.n_trees))
    pick = ids + [A.n_trees - 6, A.n_trees + 3, 2]  # three trees twice: A's deepest, one of B, a small one
    rng.shuffle(pick)
    return A, B, pick


# ---- 1. a mixed pick of two forests ----
@pytest.mark.parametrize("arity", ARITIES)
def test_mixed_pick_equals_the_gather_and_a_fresh_build(gpu_ctx, oracle_mod, arity):
    import torch
    A, B, pick = _mixed_case(gpu_ctx, oracle_mod, arity)
    assert len(pick) == 40
    cap = sum((A.sizes + B.sizes)[p] for p in pick) + 3
    M, out = _run(gpu_ctx, arity, A, B, pick, cap)
    assert M["n_bad"] == 0
    max_leaves = max(A.max_leaves, B.max_leaves)
    levels, roots, bad = _fresh_like(gpu_ctx, arity, out, len(pick), cap, max_leaves)
    assert int(bad) == 0 and torch.equal(out[2], levels) and torch.equal(out[3], roots)
    got_leaves, got_roots = _np(out[0]), _np(out[3])
    tree = _tree(oracle_mod, arity)
    for j in (0, 17, 39):
        at = int(M["offsets_new"][j])
        assert np.array_equal(got_roots[j], tree(_tag(arity), got_leaves[at:at + M["n"][j]])[0]), j


# ---- 2. the identity pick of A alone ----
@pytest.mark.parametrize("arity", ARITIES)
def test_identity_pick_reproduces_the_forest(gpu_ctx, oracle_mod, arity):
    import torch
    A = Src(gpu_ctx, oracle_mod, arity, _mix(arity) + [1] * 5, 0x5E30 + arity)
    n_leaves = sum(A.sizes)
    M, out = _run(gpu_ctx, arity, A, None, range(A.n_trees), n_leaves)
    used = int(M["level_starts"][-1])
    assert torch.equal(out[0][:n_leaves], A.d) and torch.equal(out[1][:A.n_trees + 1], A.d_off)
    assert torch.equal(out[2][:used], A.d_lv[:used]) and torch.equal(out[3][:A.n_trees], A.roots)


# ---- 3. trees that cross, fill and end on the relocation tiles ----
@pytest.mark.parametrize("arity", ARITIES)
def test_tile_edges(gpu_ctx, oracle_mod, arity):
    import torch
    tile = 512  # FOREST_SELECT_MOVE_TILE of csrc/forest_ragged.h
    for k, sizes in enumerate(([1] * 600 + [4 ** 6 + 5] + [1] * 600, [tile, 100], [3 * tile, 3], [tile - 1, 1, tile + 1, 2 * tile])):
        A = Src(gpu_ctx, oracle_mod, arity, sizes, 0x5E40 + 8 * k + arity)
        for pick in (list(range(len(sizes)))[::-1], list(range(len(sizes)))):
            M, out = _run(gpu_ctx, arity, A, None, pick, sum(sizes))
            levels, roots, bad = _fresh_like(gpu_ctx, arity, out, len(pick), sum(sizes), A.max_leaves)
            assert int(bad) == 0 and torch.equal(out[2], levels) and torch.equal(out[3], roots)


# ---- 4. refused picks ----
@pytest.mark.parametrize("arity", ARITIES)
def test_bad_picks_and_the_cap_rule(gpu_ctx, oracle_mod, arity):
    sizes_a, sizes_b = [5, 0, 40, 9, 17, 3, 1, 8], [6, 2, 11]
    A = Src(gpu_ctx, oracle_mod, arity, sizes_a, 0x5E60 + arity, max_leaves=20, bad=[2])  # tree 1 is empty, tree 2 above max_leaves
    B = Src(gpu_ctx, oracle_mod, arity, sizes_b, 0x5E68 + arity)
    assert not _np(A.roots)[1].any() and not _np(A.roots)[2].any()  # the build's own verdict
    pick = [0, 11, 1, U64_MAX, 2, 8, 3, 4, 1, 9, 5, 10, 6, 7]  # 11 = n_trees_a + n_trees_b
    cap = 5 + 6 + 9 + 17 + 2 + 3 + 4  # the last three non-empty picks (11, 1 and 8 leaves) overflow; the one-leaf tree would fit alone
    M, out = _run(gpu_ctx, arity, A, B, pick, cap)
    assert M["refused"] == [False, True, True, True, True, False, False, False, True, False, False, True, True, True] and M["n_bad"] == 8
    levels, roots, bad = _fresh_like(gpu_ctx, arity, out, len(pick), cap, 20)
    import torch
    assert int(bad) == M["n_bad"] and torch.equal(out[2], levels) and torch.equal(out[3], roots)


# ---- 5. more picks than two trips of the scan ----
@pytest.mark.parametrize("arity", ARITIES)
def test_scan_width(gpu_ctx, arity):
    import torch
    import scanwidth as SW
    assert SW.SCANS["k_fr_scan_tiles"][0] == 2048 and SW.trips("k_fr_scan_tiles", SW.WIDE_TREES) == 3  # the select scans with the build's tiles
    f = SW.wide_forest(arity)
    T, n_leaves = len(f.sizes), int(f.off[-1])
    d, d_off = _torch(f.flat), _torch(f.off.astype(np.uint64))
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, T, f.max_leaves)
    pick = torch.arange(T - 1, -1, -1, dtype=torch.int64, device="cuda:0")
    out, bad = _buffers(arity, n_leaves, T, f.max_leaves)
    bound = TS.levels_bound(n_leaves, T, f.max_leaves, arity)
    _method(gpu_ctx, arity)((d, d_off, T, f.max_leaves, d_lv, roots), None, pick, T, out[0][:n_leaves], out[1][:T + 1], out[2][:bound], out[3][:T], bad)
    sizes = _torch(f.sizes.astype(np.int64))
    new_sizes = sizes.flip(0)
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(new_sizes, 0)])
    # new leaf i lies in new tree j at i - want_off[j]; it is leaf d_off[T - 1 - j] + that of the source
    j = torch.repeat_interleave(torch.arange(T, device="cuda:0"), new_sizes)
    src = d_off[T - 1 - j] + (torch.arange(n_leaves, device="cuda:0") - want_off[j])
    assert int(bad) == 0 and torch.equal(out[1][:T + 1], want_off) and torch.equal(out[0][:n_leaves], d[src]) and torch.equal(out[3][:T], roots.flip(0))
    levels, f_roots, f_bad = _fresh_like(gpu_ctx, arity, out, T, n_leaves, f.max_leaves)
    assert int(f_bad) == 0 and torch.equal(out[2], levels) and torch.equal(out[3], f_roots)
    for t in out[:2] + out[3:]:
        assert bool((t[-TAIL:] == SENTINEL).all())


# ---- 6. 64-bit indexing ----
def test_second_tree_past_4_gib(gpu_ctx):
    import torch
    arity = 4
    n0, n1 = (1 << 27) + 8, 1000  # the second tree starts past 2^27 scalars (4 GiB) in the source; the first tree ends past them in the result
    n_leaves = n0 + n1
    bound = TS.levels_bound(n_leaves, 2, n0, arity)
    need = 2 * (n_leaves + bound) * 32 + (2 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d GiB of free HBM" % (need >> 30))
    d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(TS.offsets([n0, n1]))
    roots, d_lv = _build(gpu_ctx, arity, d, d_off, 2, n0)
    out = (torch.empty((n_leaves, 4), dtype=torch.int64, device="cuda:0"), torch.full((3 + TAIL,), SENTINEL, dtype=torch.int64, device="cuda:0"),
           torch.empty((bound, 4), dtype=torch.int64, device="cuda:0"), torch.full((2 + TAIL, 4), SENTINEL, dtype=torch.int64, device="cuda:0"))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _method(gpu_ctx, arity)((d, d_off, 2, n0, d_lv, roots), None, _torch(np.array([1, 0], np.uint64)), 2, out[0], out[1][:3], out[2], out[3][:2], bad)
    torch.cuda.synchronize()
    l0, l1 = TS.levels_len(n0, arity), TS.levels_len(n1, arity)
    assert int(bad) == 0 and out[1][:3].tolist() == [0, n1, n1 + n0] and bool((out[1][3:] == SENTINEL).all())
    assert torch.equal(out[3][:2], roots.flip(0)) and bool((out[3][2:] == SENTINEL).all())
    w = 4096
    assert torch.equal(out[0][:n1], d[n0:]) and torch.equal(out[0][n1:n1 + w], d[:w]) and torch.equal(out[0][n_leaves - w:], d[n0 - w:n0])
    assert torch.equal(out[2][:l1], d_lv[l0:l0 + l1]) and torch.equal(out[2][l1:l1 + w], d_lv[:w]) and torch.equal(out[2][l1 + l0 - w:l1 + l0], d_lv[l0 - w:l0])
    assert torch.equal(out[0][n1:], d[:n0]) and torch.equal(out[2][l1:l1 + l0], d_lv[:l0])  # and everything between
    del d, d_lv, out
    torch.cuda.empty_cache()


# ---- 7. the result is an ordinary forest ----
@pytest.mark.parametrize("arity", ARITIES)
def test_result_is_an_ordinary_forest(gpu_ctx, oracle_mod, arity):
    import torch
    A, B, pick = _mixed_case(gpu_ctx, oracle_mod, arity)
    n = len(pick)
    cap = sum((A.sizes + B.sizes)[p] for p in pick)
    max_leaves = max(A.max_leaves, B.max_leaves)
    M, out = _run(gpu_ctx, arity, A, B, pick, cap)
    bound = TS.levels_bound(cap, n, max_leaves, arity)
    sel = Grown(arity, (out[0][:cap], out[1], out[2][:bound], out[3]), n, max_leaves)
    twin_leaves = out[0][:cap].clone()
    twin_roots, twin_lv = _build(gpu_ctx, arity, twin_leaves, sel.d_off, n, max_leaves)
    twin = Grown(arity, (twin_leaves, out[1].clone(), twin_lv, twin_roots), n, max_leaves)
    # one leaf of every tree: opened, re-hashed and verified
    tid, lid = np.arange(n), np.array([(7 * j) % s for j, s in enumerate(M["n"])])
    opened = []
    for F in (sel, twin):
        o = _open(gpu_ctx, arity, F.d, F.d_off, n, max_leaves, F.d_lv, tid, lid)
        ok = _verify(gpu_ctx, arity, o, F.roots, n)
        torch.cuda.synchronize()
        assert bool((ok == 1).all()) and not bool(o["bad"].any())
        opened.append(o)
    for key in ("leaves", "sib", "pos", "dep"):
        assert torch.equal(opened[0][key], opened[1][key]), key
    # one update of a leaf in three trees
    big = int(np.argmax(M["n"]))
    trees = [big] + [t for t in (0, n - 1, 1) if t != big][:2]
    new = oracle_mod.fill_random(0x5E70 + arity, 3)
    for F in (sel, twin):
        bad, _ = _update(gpu_ctx, arity, F.d, F.d_off, n, max_leaves, F.d_lv, trees, [M["n"][t] - 1 for t in trees], new, F.roots)
        assert int(bad) == 0
    torch.cuda.synchronize()
    used = int(M["level_starts"][-1])  # (past it the select's buffer holds the sentinel, the fresh build's zeros)
    assert torch.equal(sel.d, twin.d) and torch.equal(sel.d_lv[:used], twin.d_lv[:used]) and torch.equal(sel.roots, twin.roots)
    # one append of two leaves to one tree
    add = _torch(oracle_mod.fill_random(0x5E78 + arity, 2))
    aoff = np.zeros(n + 1, np.uint64)
    aoff[6:] = 2
    grown = []
    for F in (sel, twin):
        g = _outputs(arity, cap + 2, n, max_leaves + 2)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        _append(gpu_ctx, F, add, _torch(aoff), n, max_leaves + 2, g, bad)
        torch.cuda.synchronize()
        assert int(bad) == 0
        grown.append(g)
    for got, want in zip(*grown):
        assert torch.equal(got, want)


# ---- 8. two streams of one context ----
@pytest.mark.parametrize("arity", ARITIES)
def test_two_streams_of_one_context(gpu_ctx, oracle_mod, arity):
    import torch
    A, B, pick = _mixed_case(gpu_ctx, oracle_mod, arity)
    sizes = A.sizes + B.sizes
    jobs = []
    for p in (pick, pick[::-1][:25] + [3] * 400):
        cap = sum(sizes[i] for i in p)
        M, alone = _run(gpu_ctx, arity, A, B, p, cap)
        out, _ = _buffers(arity, cap, len(p), max(A.max_leaves, B.max_leaves))
        jobs.append(dict(pick=_torch(np.asarray(p, np.uint64)), n=len(p), cap=cap, alone=alone, out=out))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")]
    for rep in range(3):
        for J, s in zip(jobs, streams):
            with torch.cuda.stream(s):
                for t in J["out"]:
                    t.fill_(SENTINEL)
                _select(gpu_ctx, arity, A, B, J["pick"], J["n"], J["cap"], J["out"], None)
        torch.cuda.synchronize()
        for J in jobs:
            for got, want in zip(J["out"], J["alone"]):
                assert torch.equal(got, want), rep


# ---- the call in a captured graph: no memset node, no allocation once the stream's scratch is warm ----
def test_graph_capture(gpu_ctx, oracle_mod):
    import torch
    arity = 4
    A, B, pick = _mixed_case(gpu_ctx, oracle_mod, arity)
    sizes = A.sizes + B.sizes
    cap = sum(sizes[i] for i in pick)
    M, alone = _run(gpu_ctx, arity, A, B, pick, cap)
    out, bad = _buffers(arity, cap, len(pick), max(A.max_leaves, B.max_leaves))
    d_pick = _torch(np.asarray(pick, np.uint64))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _select(gpu_ctx, arity, A, B, d_pick, len(pick), cap, out, bad)  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _select(gpu_ctx, arity, A, B, d_pick, len(pick), cap, out, bad)
    for t in out:
        t.fill_(SENTINEL)
    bad.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert int(bad) == 0
    for got, want in zip(out, alone):
        assert torch.equal(got, want)


# ---- 9. the host refusals, through ctypes ----
@pytest.mark.parametrize("arity", ARITIES)
def test_host_refusals(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import _lib
    fn = getattr(_lib.lib(), "p252_merkle%d_forest_ragged_select_device_into" % arity)
    A = Src(gpu_ctx, oracle_mod, arity, [5, 17, 1, 9], 0x5E80 + arity)
    B = Src(gpu_ctx, oracle_mod, arity, [3, 30], 0x5E88 + arity)
    pick = _torch(np.array([5, 0, 3, 1, 1], np.uint64))
    n_pick, cap = 5, 30 + 5 + 9 + 17 + 17 + 2
    need = TS.levels_bound(cap, n_pick, 30, arity)
    out, bad = _buffers(arity, cap, n_pick, 30)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(d_leaves_a=A.d.data_ptr(), n_leaves_a=sum(A.sizes), d_offsets_a=A.d_off.data_ptr(), n_trees_a=4, max_leaves_a=17, d_levels_a=A.d_lv.data_ptr(),
                d_roots_a=A.roots.data_ptr(), d_leaves_b=B.d.data_ptr(), n_leaves_b=sum(B.sizes), d_offsets_b=B.d_off.data_ptr(), n_trees_b=2,
                max_leaves_b=30, d_levels_b=B.d_lv.data_ptr(), d_roots_b=B.roots.data_ptr(), d_pick=pick.data_ptr(), n_pick=n_pick,
                d_leaves_new=out[0].data_ptr(), leaves_cap=cap, d_offsets_new=out[1].data_ptr(), d_levels_new=out[2].data_ptr(), levels_cap=need,
                d_roots_new=out[3].data_ptr(), d_n_bad=bad.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return fn(gpu_ctx._h, *[a[k] for k in base], stream)

    def refused(word, **kw):
        rc = call(**kw)
        msg = _lib.lib().p252_last_error(gpu_ctx._h).decode()
        assert rc == _lib.ERR_INVALID_ARGUMENT and word in msg, (kw, rc, msg)
    assert call() == _lib.OK  # the control; levels_cap is the bound itself
    torch.cuda.synchronize()
    assert int(bad) == 0 and out[1][:n_pick + 1].tolist() == [0, 30, 35, 44, 61, 78]
    for name in ("d_leaves_a", "d_offsets_a", "d_levels_a", "d_roots_a", "d_leaves_b", "d_offsets_b", "d_levels_b", "d_roots_b", "d_pick", "d_leaves_new",
                 "d_offsets_new", "d_levels_new", "d_roots_new"):
        refused("NULL", **{name: None})
    assert call(d_n_bad=None) == _lib.OK
    for name in ("d_leaves_a", "d_levels_a", "d_roots_a", "d_leaves_b", "d_levels_b", "d_roots_b", "d_leaves_new", "d_levels_new", "d_roots_new"):
        refused("16-byte aligned", **{name: base[name] + 8})
    for name in ("d_offsets_a", "d_offsets_b", "d_pick", "d_offsets_new"):
        refused("8-byte aligned", **{name: base[name] + 4})
    refused("4-byte aligned", d_n_bad=base["d_n_bad"] + 2)
    refused("n_trees_a", n_trees_a=0)
    refused("leaves_cap", leaves_cap=0)
    refused("levels_cap", levels_cap=need - 1)
    refused("size overflow", n_pick=2 ** 64 // 8 // 66 + 1)
    refused("size overflow", n_leaves_a=2 ** 64 // 64 + 1)
    refused("d_leaves_new overlaps d_leaves_a", d_leaves_new=base["d_leaves_a"] + 32 * (sum(A.sizes) - 1))
    refused("d_roots_new overlaps d_pick", d_roots_new=base["d_pick"] + 16)
    refused("d_offsets_new overlaps d_leaves_new", d_offsets_new=base["d_leaves_new"] + 64)
    assert call(n_pick=0) == _lib.OK
    # B absent: its six other arguments may be 0 / NULL
    only_a = _torch(np.array([3, 0], np.uint64))
    assert call(d_leaves_b=None, n_leaves_b=0, d_offsets_b=None, n_trees_b=0, max_leaves_b=0, d_levels_b=None, d_roots_b=None, d_pick=only_a.data_ptr(),
                n_pick=2) == _lib.OK
    torch.cuda.synchronize()
    assert out[1][:3].tolist() == [0, 9, 14]
    # max_leaves <= 1 on both sides: no level anywhere, d_levels_x and d_levels_new may be NULL
    ones = Src(gpu_ctx, oracle_mod, arity, [1, 1, 1], 0x5E90 + arity)
    assert call(d_leaves_a=ones.d.data_ptr(), n_leaves_a=3, d_offsets_a=ones.d_off.data_ptr(), n_trees_a=3, max_leaves_a=1, d_levels_a=None,
                d_roots_a=ones.roots.data_ptr(), d_leaves_b=None, n_leaves_b=0, d_offsets_b=None, n_trees_b=0, max_leaves_b=0, d_levels_b=None,
                d_roots_b=None, d_pick=only_a.data_ptr(), n_pick=2, d_levels_new=None) == _lib.OK
    torch.cuda.synchronize()
    assert out[1][:3].tolist() == [0, 0, 1] and torch.equal(out[0][:1], ones.d[:1]) and int(bad) == 1  # id 3 is out of range there


# ---- merkle.forest_ragged_select: the outputs sized and allocated by the binding ----
@pytest.mark.parametrize("arity", ARITIES)
def test_python_helper_allocates_the_new_forest(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import merkle
    A, B, pick = _mixed_case(gpu_ctx, oracle_mod, arity)
    pick = list(dict.fromkeys(pick))[:12] + [A.n_trees + B.n_trees]  # no tree twice here: the default capacity, the leaves of both sources, is enough; one id names no tree
    M = FS.select_model(arity, A.sizes, A.bad, B.sizes, B.bad, pick, sum(A.sizes) + sum(B.sizes))
    leaves, off, levels, roots, bad = merkle.forest_ragged_select(gpu_ctx, A.view(), pick, B.view(), arity=arity)
    torch.cuda.synchronize()
    want_leaves, want_levels, want_roots = FS.gather(M, arity, A.host(), B.host())
    assert leaves.shape[0] == sum(A.sizes) + sum(B.sizes) and levels.shape[0] == TS.levels_bound(leaves.shape[0], len(pick), max(A.max_leaves, B.max_leaves), arity)
    assert int(bad) == 1 and np.array_equal(_np(off), M["offsets_new"]) and np.array_equal(_np(roots), want_roots)
    assert np.array_equal(_np(leaves)[:want_leaves.shape[0]], want_leaves) and np.array_equal(_np(levels)[:want_levels.shape[0]], want_levels)
    only_a = merkle.forest_ragged_select(gpu_ctx, A.view(), np.array([1, 0]), arity=arity)
    torch.cuda.synchronize()
    assert _np(only_a[1]).tolist() == [0, A.sizes[1], A.sizes[1] + A.sizes[0]] and torch.equal(only_a[3], A.roots[:2].flip(0)) and int(only_a[4]) == 0


# ---- 10. the C++ mirror ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    assert "ALL PASSED" in run_cpp_mirror(build_cpp_mirror("test_forest_select_api", tmp_path))


# ---- 11. the bench tool ----
# The floor on the select's bytes per second over a hipMemcpyDtoDAsync's of the same bytes in the same run, for the permutation pick of the
# 20,000-tree mixed forest: the ratio first measured on an MI355X (profiles/forest_select.txt, "mixed arity 4, permutation": RATIO_MEASURED)
# less 15 %, the margin tests/test_ragged_gpu.py gives same-run ratios.
RATIO_MEASURED = 0.775
RATE_OVER_COPY_FLOOR = 0.65  # 0.775 * 0.85 = 0.659, rounded down


def test_bench_tool_select_beats_a_rebuild_and_keeps_its_rate(gpu_ctx, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "forest_select_bench.py"), "--reps", "20", "--cases", "mixed", "--out",
                        str(tmp_path / "forest_select.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    picks = res["cases"]["mixed"]["picks"]
    assert set(picks) == {"identity", "1 % dropped", "permutation", "merge of two halves"}
    for name, p in picks.items():
        print("%s: select %.3f ms, fresh build %.3f ms, copy %.3f ms, rate over copy %.3f" % (name, p["select_ms"], p["rebuild_ms"], p["copy_ms"],
                                                                                             p["rate_over_copy"]))
        assert p["outputs_equal"], name
        assert p["select_ms"] < p["rebuild_ms"], (name, p)  # a condition, not a measurement: the select hashes nothing
    assert picks["permutation"]["rate_over_copy"] >= RATE_OVER_COPY_FLOOR, picks["permutation"]
