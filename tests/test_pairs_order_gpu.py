"""The order and the distinct (tree id, leaf id) pairs made on the device (p252_pairs_order_device_into, p252_pairs_unique_device_into;
csrc/pairs.hip) on the GPU.  Every comparison is exact equality with the numpy model (testsupport/pairsmodel.py): the order is a unique
permutation, so there is no tolerance anywhere.  The sizes hang on the constants of csrc/pairs.h: around a wave, around a tile, several
tiles, and the smallest k that takes the trips of both scans over the tiles (k_po_scan, k_po_scan_heads) into their second
iteration, plus one tile and 3.  Outputs live in sentinel-filled buffers with one entry behind them, which must keep the sentinel."""
import os
import re

import numpy as np
import pytest

from helpers.forest import SENTINEL, _forest, _np, _tag, _torch
from testsupport import forestsequential as FS
from testsupport import pairsmodel as PM
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "poseidon252_amd", "csrc", "pairs.h")).read()
C = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*constexpr unsigned\s+(PAIRS_\w+)\s*=\s*(\d+)u?\s*;", _H, re.M)}
TILE, SCAN = C["PAIRS_TILE"], C["PAIRS_SCAN_BLOCK"]
# the scans over the tiles take SCAN tiles a trip: SCAN * TILE + 1 pairs are SCAN + 1 tiles, the first of a second trip
WIDE = SCAN * TILE + 1 + TILE + 3
assert WIDE <= 1 << 22
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, WIDE]
SENT32, SENT64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)
FOREST_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257]


# ---- the key patterns: (rng, k) -> (tree ids uint32 or None, leaf ids uint64) ----
def _equal(rng, k):
    return np.full(k, 7, np.uint32), np.full(k, 3, np.uint64)


def _alternating(rng, k):
    return np.full(k, 1, np.uint32), np.where(np.arange(k) % 2 == 0, 5, 2).astype(np.uint64)


def _sorted(rng, k):  # strictly ascending: all distinct
    return (np.arange(k) >> 10).astype(np.uint32), (np.arange(k, dtype=np.uint64) * np.uint64(3))


def _reversed(rng, k):
    t, j = _sorted(rng, k)
    return t[::-1].copy(), j[::-1].copy()


def _half_repeats(rng, k):
    """tree ids below 2^16, leaf ids below 2^24; about half the pairs repeat an earlier original"""
    t, j = rng.integers(0, 1 << 16, k).astype(np.uint32), rng.integers(0, 1 << 24, k).astype(np.uint64)
    original = rng.random(k) < 0.5
    original[0] = True
    originals = np.nonzero(original)[0]
    before = np.cumsum(original) - original  # originals before i (> 0 for every repeat)
    rep = np.nonzero(~original)[0]
    src = originals[(rng.random(rep.size) * before[rep]).astype(np.int64)]
    assert (src < rep).all()
    t[rep], j[rep] = t[src], j[src]
    return t, j


def _byte(b):
    def make(rng, k):
        """keys that differ in byte b only: pass b runs alone, every other one is skipped"""
        vals = rng.integers(0, 256, k).astype(np.uint64)
        if b < 8:
            return np.full(k, 0x01020304, np.uint32), (vals << np.uint64(8 * b)) | np.uint64(0x1112131415161718 & ~(0xFF << (8 * b)))
        return ((vals << np.uint64(8 * (b - 8))).astype(np.uint32) | np.uint32(0x01020304 & ~(0xFF << (8 * (b - 8))))), np.full(k, 0x1112131415161718, np.uint64)
    return make


def _bytes_0_and_11(rng, k):
    return (rng.integers(0, 256, k).astype(np.uint64) << np.uint64(24)).astype(np.uint32), rng.integers(0, 256, k).astype(np.uint64) | np.uint64(0x7700)


def _extremes(rng, k):
    t = np.array([0xFFFFFFFF, 0, 0x80000000, 0x7FFFFFFF], np.uint32)[rng.integers(0, 4, k)]
    j = np.array([2 ** 63, 2 ** 64 - 1, 0, 1, 2 ** 63 - 1], np.uint64)[rng.integers(0, 5, k)]
    return t, j


def _no_trees(rng, k):
    return None, rng.integers(0, 1 << 20, k).astype(np.uint64)


PATTERNS = dict([("equal", _equal), ("alternating", _alternating), ("sorted", _sorted), ("reversed", _reversed), ("half_repeats", _half_repeats)] +
                [("byte%d" % b, _byte(b)) for b in range(12)] + [("bytes_0_and_11", _bytes_0_and_11), ("extremes", _extremes), ("no_trees", _no_trees)])


# ---- the calls, into sentinel-filled buffers with one entry behind ----
def _order(ctx, d_t, d_j, k, stream=None):
    import torch
    out = torch.full((k + 1,), int(np.int32(SENT32.view(np.int32))), dtype=torch.int32, device=d_j.device)
    ctx.pairs_order_device(d_t, d_j, k, out, stream=stream)
    return out


def _order_result(out):
    a = out.cpu().numpy().view(np.uint32)
    assert a[-1] == SENT32
    return a[:-1]


def _unique(ctx, d_t, d_j, k, outputs=("t", "j", "i", "f")):
    import torch
    s32, s64 = int(SENT32.view(np.int32)), int(SENT64.view(np.int64))
    b = dict(t=torch.full((k + 1,), s32, dtype=torch.int32, device=d_j.device), j=torch.full((k + 1,), s64, dtype=torch.int64, device=d_j.device),
             i=torch.full((k + 1,), s32, dtype=torch.int32, device=d_j.device), f=torch.full((k + 1,), s32, dtype=torch.int32, device=d_j.device),
             n=torch.full((1,), -1, dtype=torch.int64, device=d_j.device))
    give = lambda name: b[name] if name in outputs else None  # noqa: E731
    ctx.pairs_unique_device(d_t, d_j, k, b["n"], d_tree_ids_out=give("t"), d_leaf_ids_out=give("j"), d_indices_out=give("i"), d_first=give("f"))
    return b


def _unique_result(b, outputs=("t", "j", "i", "f")):
    """-> (n, t, j, indices, first), each cut at n; everything at and past n keeps the sentinel, and so does an output not given"""
    n = int(b["n"])
    got = {}
    for name in ("t", "j", "i", "f"):
        a = b[name].cpu().numpy()
        a = a.view(np.uint64) if name == "j" else a.view(np.uint32)
        sent = SENT64 if name == "j" else SENT32
        assert (a[n if name in outputs else 0:] == sent).all(), name
        got[name] = a[:n]
    return n, got["t"], got["j"], got["i"], got["f"]


def _dev(t, j):
    return (None if t is None else _torch(t)), _torch(j)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_every_size_of_a_key_pattern_equals_the_model(gpu_ctx, pattern):
    import torch
    rng = np.random.default_rng([0x9A125, list(PATTERNS).index(pattern)])
    for k in SIZES:
        t, j = PATTERNS[pattern](rng, k)
        d_t, d_j = _dev(t, j)
        o, u = _order(gpu_ctx, d_t, d_j, k), _unique(gpu_ctx, d_t, d_j, k)
        torch.cuda.synchronize()
        order = _order_result(o)
        want = PM.order(t, j)
        assert np.array_equal(order, want), (pattern, k)
        wt, wj, wf = PM.unique(t, j)
        n, gt, gj, gi, gf = _unique_result(u)
        assert n == wt.size, (pattern, k, n)
        assert np.array_equal(gt, wt) and np.array_equal(gj, wj) and np.array_equal(gi, wj.astype(np.uint32)) and np.array_equal(gf, wf), (pattern, k)
        if pattern == "equal":
            assert order.tolist() == list(range(k)) if k < 100 else np.array_equal(order, np.arange(k))  # pure stability: the identity
            assert n == 1 and gf.tolist() == [0]
        if pattern in ("sorted", "reversed"):
            assert n == k  # all distinct
            assert np.array_equal(order, np.arange(k) if pattern == "sorted" else np.arange(k)[::-1])
        if pattern == "no_trees":  # None is an explicit array of zeros
            z = _torch(np.zeros(k, np.uint32))
            o2, u2 = _order(gpu_ctx, z, d_j, k), _unique(gpu_ctx, z, d_j, k)
            torch.cuda.synchronize()
            assert np.array_equal(_order_result(o2), order)
            n2, t2, j2, i2, f2 = _unique_result(u2)
            assert n2 == n and np.array_equal(j2, gj) and np.array_equal(f2, gf) and not t2.any() and not gt.any()
        if re.fullmatch(r"byte\d+", pattern):
            b = int(pattern[4:])  # that pass alone (pass 0 where the byte happens to hold one value, as at k = 1)
            assert PM.varying_passes(t, j) == ([b] if np.unique(PM.digit(t, j, b)).size > 1 else [0])
    if pattern == "half_repeats":  # the model of the device's method, at the device's tile, says the same (once, at the several-tile size)
        t, j = PATTERNS[pattern](np.random.default_rng(5), 3 * TILE + 5)
        assert np.array_equal(PM.device_order(t, j, tile=TILE)[0], PM.order(t, j))


def test_unique_writes_only_the_outputs_it_is_given(gpu_ctx):
    import torch
    rng = np.random.default_rng(77)
    k = TILE + 1
    t, j = _half_repeats(rng, k)
    d_t, d_j = _dev(t, j)
    wt, wj, wf = PM.unique(t, j)
    for outputs in (("f",), ("i",), ("t", "j"), ("j", "f")):
        u = _unique(gpu_ctx, d_t, d_j, k, outputs)
        torch.cuda.synchronize()
        n, gt, gj, gi, gf = _unique_result(u, outputs)
        assert n == wt.size
        for name, got, want in (("t", gt, wt), ("j", gj, wj), ("i", gi, wj.astype(np.uint32)), ("f", gf, wf)):
            if name in outputs:
                assert np.array_equal(got, want), (outputs, name)


def test_the_helpers_return_the_models_tensors(gpu_ctx):
    import torch
    from poseidon252_amd import merkle
    rng = np.random.default_rng(3)
    t, j = _extremes(rng, 500)
    order = merkle.pairs_order(t, j, ctx=gpu_ctx)
    assert order.dtype == torch.int32 and order.is_cuda and np.array_equal(order.cpu().numpy().view(np.uint32), PM.order(t, j))
    ut, uj, first = merkle.pairs_unique(t, j, ctx=gpu_ctx)
    wt, wj, wf = PM.unique(t, j)
    assert ut.dtype == torch.int32 and uj.dtype == torch.int64 and first.dtype == torch.int32
    assert np.array_equal(ut.cpu().numpy().view(np.uint32), wt) and np.array_equal(_np(uj), wj) and np.array_equal(first.cpu().numpy().view(np.uint32), wf)
    lone = merkle.pairs_order(None, [5, 3, 5, 0], ctx=gpu_ctx)
    assert lone.tolist() == [3, 1, 0, 2]
    ut, uj, first = merkle.pairs_unique(None, torch.tensor([5, 3, 5, 0]), ctx=gpu_ctx)
    assert ut.tolist() == [0, 0, 0] and uj.tolist() == [0, 3, 5] and first.tolist() == [3, 1, 0]
    with pytest.raises(ValueError, match="no pairs"):
        merkle.pairs_order([], [], ctx=gpu_ctx)
    with pytest.raises(ValueError, match="3 tree ids, 2 leaf ids"):
        merkle.pairs_unique([0, 1, 2], [0, 1], ctx=gpu_ctx)


# ---- into the consumers, on small forests ----
def _small_forest(gpu_ctx, arity, seed):
    off = TS.offsets(FOREST_SIZES)
    flat = np.random.default_rng(seed).integers(0, 1 << 60, size=(int(off[-1]), 4), dtype=np.uint64)
    return off, flat, _forest(gpu_ctx, arity, flat, off)


def _pairs_in_forest(rng, k):
    sizes = np.asarray(FOREST_SIZES)
    t = rng.integers(0, sizes.size, k)
    j = (rng.random(k) * sizes[t]).astype(np.int64)
    rep = np.nonzero(rng.random(k) < 0.5)[0]
    rep = rep[rep > 0]
    src = (rng.random(rep.size) * rep).astype(np.int64)
    t[rep], j[rep] = t[src], j[src]  # (an earlier place, as first drawn)
    return t.astype(np.uint32), j.astype(np.uint64)


@pytest.mark.parametrize("arity", [4, 2])
def test_the_librarys_order_goes_into_the_sequential_update(gpu_ctx, arity):
    import torch
    k = 300
    t, j = _pairs_in_forest(np.random.default_rng(40 + arity), k)
    new = np.random.default_rng(50 + arity).integers(0, 1 << 60, size=(k, 4), dtype=np.uint64)
    D, per, T, top = int(TS.depth(max(FOREST_SIZES), arity)), arity - 1, len(FOREST_SIZES), max(FOREST_SIZES)
    d_t, d_j, d_new = _torch(t), _torch(j), _torch(new)
    results = []
    for route in ("library", "model"):
        off, flat, (d, d_off, roots, d_lv) = _small_forest(gpu_ctx, arity, 60 + arity)
        if route == "library":
            d_order = _order(gpu_ctx, d_t, d_j, k)[:k]
        else:
            d_order = _torch(FS.stable_order(t, j))
        full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device=d.device)  # noqa: E731
        b = dict(old=full(k, 4), before=full(k, 4), after=full(k, 4), sib=full(k, D, per, 4), pos=torch.full((k, D), 7, dtype=torch.uint8, device=d.device),
                 dep=torch.full((k,), 7, dtype=torch.uint8, device=d.device), bad=torch.zeros(1, dtype=torch.int32, device=d.device))
        call = gpu_ctx.merkle4_forest_ragged_update_sequential_device if arity == 4 else gpu_ctx.merkle2_forest_ragged_update_sequential_device
        call(_tag(arity), d, d_off, T, top, d_lv, d_t, d_j, d_new, d_order.contiguous(), k, b["sib"], b["pos"], b["dep"], b["after"], d_old_leaves=b["old"],
             d_roots_before=b["before"], d_roots=roots, d_n_bad=b["bad"])
        torch.cuda.synchronize()
        assert int(b["bad"]) == 0, route
        results.append([x.cpu().numpy() for x in (d_order, b["old"], b["before"], b["after"], b["sib"], b["pos"], b["dep"], d, d_lv, roots)])
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    assert (results[0][6] != 0xFF).all()


@pytest.mark.parametrize("arity", [4, 2])
def test_the_distinct_pairs_go_into_the_forests_shared_proof(gpu_ctx, arity):
    import torch
    k = 300
    t, j = _pairs_in_forest(np.random.default_rng(70 + arity), k)
    off, flat, (d, d_off, roots, d_lv) = _small_forest(gpu_ctx, arity, 80 + arity)
    T, top = len(FOREST_SIZES), max(FOREST_SIZES)
    u = _unique(gpu_ctx, _torch(t), _torch(j), k)
    torch.cuda.synchronize()
    n = _unique_result(u)[0]
    wt, wj, _ = PM.unique(t, j)
    assert n == wt.size
    bound = gpu_ctx.merkle_forest_ragged_multiproof_bound(flat.shape[0], T, top, n, arity=arity)
    proofs = []
    for d_tid, d_lid in ((u["t"][:n].contiguous(), u["j"][:n].contiguous()), (_torch(wt), _torch(wj))):
        out = torch.full((n, 4), SENTINEL, dtype=torch.int64, device=d.device)
        proof = torch.full((bound, 4), SENTINEL, dtype=torch.int64, device=d.device)
        po = torch.full((T + 1,), -1, dtype=torch.int64, device=d.device)
        bad = torch.zeros(1, dtype=torch.int32, device=d.device)
        gpu_ctx.merkle_forest_ragged_multiproof_device(d, d_off, T, top, d_lv, d_tid, d_lid, n, out, proof, po, bad, arity=arity)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(po[-1]) > 0
        proofs.append((_np(out), _np(proof), _np(po)))
    for x, y in zip(*proofs):
        assert np.array_equal(x, y)
    assert np.array_equal(proofs[0][0], flat[off[wt.astype(np.int64)].astype(np.int64) + wj.astype(np.int64)])


@pytest.mark.parametrize("arity", [4, 2])
def test_the_low_words_go_into_a_single_trees_shared_proof(gpu_ctx, arity):
    import torch
    n_leaves, k = 257, 200
    rng = np.random.default_rng(90 + arity)
    flat = rng.integers(0, 1 << 60, size=(n_leaves, 4), dtype=np.uint64)
    pos = rng.integers(0, n_leaves, k).astype(np.uint64)
    d = _torch(flat)
    _, levels = (gpu_ctx.merkle4_tree if arity == 4 else gpu_ctx.merkle2_tree)(_tag(arity), flat, want_levels=True)
    d_lv = _torch(levels)
    u = _unique(gpu_ctx, None, _torch(pos), k, outputs=("i",))
    torch.cuda.synchronize()
    n = int(u["n"])
    want = np.unique(pos)
    assert n == want.size
    bound = gpu_ctx.merkle_multiproof_bound(n_leaves, n, arity)
    proofs = []
    for d_idx in (u["i"][:n].contiguous(), _torch(want.astype(np.uint32))):
        out = torch.full((n, 4), SENTINEL, dtype=torch.int64, device=d.device)
        proof = torch.full((bound, 4), SENTINEL, dtype=torch.int64, device=d.device)
        plen = torch.full((1,), -1, dtype=torch.int64, device=d.device)
        bad = torch.zeros(1, dtype=torch.int32, device=d.device)
        gpu_ctx.merkle_multiproof_device(d, n_leaves, d_lv, d_idx, n, out, proof, plen, d_n_bad=bad, arity=arity)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(plen) > 0
        proofs.append((_np(out), _np(proof), int(plen)))
    assert np.array_equal(proofs[0][0], proofs[1][0]) and np.array_equal(proofs[0][1], proofs[1][1]) and proofs[0][2] == proofs[1][2]
    assert np.array_equal(proofs[0][0], flat[want.astype(np.int64)])


# ---- streams and graphs ----
def test_two_streams_of_one_context_sort_different_inputs_at_once(gpu_ctx):
    import torch
    k = 3 * TILE + 5
    inputs = [_half_repeats(np.random.default_rng(11), k), _extremes(np.random.default_rng(12), k)]
    dev = [_dev(t, j) for t, j in inputs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [[], []]
    for _ in range(3):  # both streams hold work at the same time: the calls return before their launches have run
        for s, (d_t, d_j), o in zip(streams, dev, outs):
            with torch.cuda.stream(s):
                o.append((_order(gpu_ctx, d_t, d_j, k), _unique(gpu_ctx, d_t, d_j, k)))
    torch.cuda.synchronize()
    for (t, j), o in zip(inputs, outs):
        want, (wt, wj, wf) = PM.order(t, j), PM.unique(t, j)
        for order, u in o:
            assert np.array_equal(_order_result(order), want)
            n, gt, gj, _, gf = _unique_result(u)
            assert n == wt.size and np.array_equal(gt, wt) and np.array_equal(gj, wj) and np.array_equal(gf, wf)


def test_a_captured_order_replays_on_other_keys_with_other_passes(gpu_ctx):
    """one capture of pairs_order_device — one stream, no fork: a linear chain of a memset and the kernels — replayed after the input
    buffers were refilled: the capture saw leaf ids below 2^16 (passes 0 and 1 run), the first refill varies in byte 2 of the leaf id and
    byte 0 of the tree id (passes 2 and 8: an even number again, but other arrays hold other records), the second in three bytes (an odd
    number of passes: the last pass reads the other array), the third is all equal (pass 0 alone, the identity)"""
    import torch
    k = 3 * TILE + 5
    rng = np.random.default_rng(21)
    t0, j0 = np.zeros(k, np.uint32), rng.integers(0, 1 << 16, k).astype(np.uint64)
    d_t, d_j = _torch(t0), _torch(j0)
    s = torch.cuda.Stream()
    out = torch.full((k + 1,), -1, dtype=torch.int32, device=d_j.device)
    with torch.cuda.stream(s):
        gpu_ctx.pairs_order_device(d_t, d_j, k, out)  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:k], PM.order(t0, j0))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gpu_ctx.pairs_order_device(d_t, d_j, k, out)
    refills = [(rng.integers(0, 256, k).astype(np.uint32), rng.integers(0, 256, k).astype(np.uint64) << np.uint64(16)),
               (rng.integers(0, 256, k).astype(np.uint32) << np.uint32(8), rng.integers(0, 1 << 16, k).astype(np.uint64) << np.uint64(40)),
               (np.full(k, 9, np.uint32), np.full(k, 1 << 63, np.uint64))]
    assert [len(PM.varying_passes(t, j)) for t, j in [(t0, j0)] + refills] == [2, 2, 3, 1]
    for t, j in refills:
        d_t.copy_(_torch(t)), d_j.copy_(_torch(j))
        out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:k], PM.order(t, j)) and got[k] == 0xFFFFFFFF


def test_cpp_mirror_runs(gpu_ctx, tmp_path, oracle_mod):
    from helpers.percall import build_cpp_mirror, run_cpp_mirror
    assert run_cpp_mirror(build_cpp_mirror("test_pairs_order_api", tmp_path)).strip().endswith("ok")
