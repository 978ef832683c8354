"""Messages of different lengths in one call (p252_hash_ragged*, csrc/ragged.hip) on the GPU, checked against the oracle's sponge
run per length (oracle.hash_batch over the messages of one length, with that length's tag)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.percall import build_cpp_mirror, run_cpp_mirror

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS_MIX = list(range(1, 10)) + [16, 41, 42, 64, 257, 1000]


def _messages(seed, lens, oracle_mod):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=off[1:])
    return oracle_mod.fill_random(seed, int(off[-1])), off


def _oracle(oracle_mod, flat, off, out_len, rows=None, domain=3):
    """digests of messages `rows` (default: all), the oracle run once per distinct length"""
    lens = (off[1:] - off[:-1]).astype(np.int64)
    rows = np.arange(lens.size) if rows is None else np.asarray(rows)
    out = np.zeros((rows.size, out_len, 4), dtype=np.uint64)
    for L in np.unique(lens[rows]):
        sel = np.nonzero(lens[rows] == L)[0]
        x = np.stack([flat[int(off[r]):int(off[r]) + int(L)] for r in rows[sel]])
        out[sel] = oracle_mod.hash_batch(oracle_mod.tag(domain, [int(L)], out_len), x, int(L), out_len, threads=8)
    return out


def _child(tmp_path, env, code):
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("out_len", [1, 3, 5, 9])
def test_mixed_lengths_match_the_oracle(gpu_ctx, oracle_mod, out_len):
    import poseidon252_amd as P
    lens = LENS_MIX * 3
    np.random.default_rng(out_len).shuffle(lens)
    flat, off = _messages(40 + out_len, lens, oracle_mod)
    exp = _oracle(oracle_mod, flat, off, out_len)
    rb = P.RaggedHashBatch(P.Domain.Other, output_len=out_len, ctx=gpu_ctx)
    got = rb.digest((flat, off))
    assert got.shape == (len(lens), out_len, 4) and np.array_equal(got, exp)
    msgs = [flat[int(off[i]):int(off[i + 1])] for i in range(len(lens))]
    assert np.array_equal(rb.digest(msgs), exp)  # the list form
    tr = rb.digest_truncated(msgs)
    assert np.array_equal(tr, P.truncate250(exp))
    # the device path, and the one-lane kernel: the same messages repeated past the lane-group switch (8,192)
    import torch
    reps = 8200 // len(lens) + 1
    big_lens = lens * reps
    big_off = np.zeros(len(big_lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(big_lens, dtype=np.uint64), out=big_off[1:])
    big_flat = np.concatenate([flat] * reps)
    d = torch.from_numpy(big_flat.view(np.int64)).cuda()
    d_off = torch.from_numpy(big_off.view(np.int64)).cuda()
    for truncated in (False, True):
        g = rb.digest((d, d_off), max_len=1000, truncated=truncated).cpu().numpy().view(np.uint64)
        want = P.truncate250(exp) if truncated else exp
        assert np.array_equal(g.reshape(reps, len(lens), out_len, 4), np.broadcast_to(want, (reps,) + want.shape)), truncated


def test_encryption_domain_tags(gpu_ctx, oracle_mod):
    import poseidon252_amd as P
    lens = [1, 2, 5, 21, 42]
    flat, off = _messages(77, lens, oracle_mod)
    got = P.RaggedHashBatch(P.Domain.Encryption, ctx=gpu_ctx).digest((flat, off))
    assert np.array_equal(got, _oracle(oracle_mod, flat, off, 1, domain=2))


_SIZES = (1, 7, 8192, 8193, 16385, 1 << 20)
_SIZES_CODE = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import poseidon252_amd as P
from poseidon252_amd import synth
rb = P.RaggedHashBatch(P.Domain.Other, output_len=%d, ctx=P.Context(0))
for n in %r:
    lens = np.random.default_rng(n).integers(1, 43, size=n).astype(np.uint64)
    off = np.zeros(n + 1, np.uint64); np.cumsum(lens, out=off[1:])
    d = synth.splitmix_scalars(1000 + n, int(off[-1]), "cuda:0")
    out = rb.digest((d, torch.from_numpy(off.view(np.int64)).cuda()), max_len=42)
    np.save("%s_%%d.npy" %% n, out.cpu().numpy())
print("done")
"""


@pytest.mark.parametrize("out_len", [1, 5])
def test_sizes_across_the_lane_group_switch_and_schedules(gpu_ctx, oracle_mod, tmp_path, out_len):
    """n on both sides of the lane-group switch; the same bytes under P252_RAGGED_SORT=0 and under P252_COOP_MAX_NODES=0 (both read
    once per process: child processes), and equal to the oracle (all messages up to 16,385; every 97th of 2^20)"""
    import torch
    from poseidon252_amd import synth
    outs = {}
    for label, env in (("default", {}), ("unsorted", {"P252_RAGGED_SORT": "0"}), ("one_lane", {"P252_COOP_MAX_NODES": "0"})):
        prefix = str(tmp_path / label)
        _child(tmp_path, env, _SIZES_CODE % (ROOT, out_len, _SIZES, prefix))
        outs[label] = {n: np.load("%s_%d.npy" % (prefix, n)) for n in _SIZES}
    for n in _SIZES:
        a = outs["default"][n]
        assert np.array_equal(a, outs["unsorted"][n]) and np.array_equal(a, outs["one_lane"][n]), n
        lens = np.random.default_rng(n).integers(1, 43, size=n).astype(np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        flat = synth.splitmix_scalars(1000 + n, int(off[-1]), "cuda:0").cpu().numpy().view(np.uint64)
        rows = np.arange(n) if n <= 16385 else np.arange(0, n, 97)
        assert np.array_equal(a.view(np.uint64)[rows], _oracle(oracle_mod, flat, off, out_len, rows)), n


@pytest.mark.parametrize("n_valid_pad", [0, 9000])
def test_bad_messages_are_zero_and_counted(gpu_ctx, oracle_mod, n_valid_pad):
    """zero-length messages, lengths above max_len and a decreasing offset pair: zero rows, d_n_bad = their count exactly, every
    valid row as the oracle's (both kernel families: with 9,000 more valid messages the one-lane kernel runs)"""
    import torch
    import poseidon252_amd as P
    max_len = 42
    lens = [5, 0, 42, 43, 7, 3, 100, 1, 3] + [int(x) for x in np.random.default_rng(3).integers(1, 43, size=n_valid_pad)]
    flat, off = _messages(91, lens, oracle_mod)
    # message 4 becomes a decreasing pair (its end moves 2 scalars before its start); message 5 grows to 7 + 2 + 3 = 12 and stays valid
    off[5] = off[4] - 2
    off_lens = off[1:].astype(np.int64) - off[:-1].astype(np.int64)
    bad = (off_lens <= 0) | (off_lens > max_len)
    assert list(np.nonzero(bad)[0]) == [1, 3, 4, 6] and off_lens[5] == 12  # empty, 43 > max_len, decreasing, 100 > max_len
    d = torch.from_numpy(flat.view(np.int64)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    rb = P.RaggedHashBatch(P.Domain.Other, output_len=3, ctx=gpu_ctx)
    got = rb.digest((d, d_off), max_len=max_len, d_n_bad=d_bad).cpu().numpy().view(np.uint64)
    assert int(d_bad.item()) == int(bad.sum())
    assert not got[bad].any()
    valid = np.nonzero(~bad)[0]
    assert np.array_equal(got[valid], _oracle(oracle_mod, flat, off, 3, valid))
    d_bad.zero_()
    got_t = rb.digest_truncated((d, d_off), max_len=max_len, d_n_bad=d_bad).cpu().numpy().view(np.uint64)
    assert int(d_bad.item()) == int(bad.sum()) and not got_t[bad].any() and np.array_equal(got_t[valid], P.truncate250(got[valid]))


def test_host_variant_error_codes(gpu_ctx, oracle_mod):
    import ctypes
    from poseidon252_amd import _lib
    L = _lib.lib()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    flat = oracle_mod.fill_random(5, 16)
    tags = np.stack([oracle_mod.tag(3, [i], 1) for i in range(1, 9)])
    out = np.zeros((3, 1, 4), np.uint64)

    def call(offsets, max_len=8, out_len=1, n=None):
        o = np.asarray(offsets, np.uint64)
        return L.p252_hash_ragged(gpu_ctx._h, tags.ctypes.data_as(u64p), max_len, flat.ctypes.data_as(u64p), o.ctypes.data_as(u64p),
                                  out_len, out.ctypes.data_as(u64p), o.size - 1 if n is None else n)
    assert call([0, 3, 5, 8]) == _lib.OK
    assert np.array_equal(out[1], _oracle(oracle_mod, flat, np.array([0, 3, 5, 8], np.uint64), 1)[1])
    assert call([0, 3, 3, 8]) == _lib.ERR_INVALID_IO_PATTERN and "empty" in L.p252_last_error(gpu_ctx._h).decode()
    assert call([0, 5, 3, 8]) == _lib.ERR_INVALID_ARGUMENT and "decrease" in L.p252_last_error(gpu_ctx._h).decode()
    assert call([0, 3, 12, 14]) == _lib.ERR_INVALID_ARGUMENT and "max_len" in L.p252_last_error(gpu_ctx._h).decode()
    assert call([0, 3, 5, 8], out_len=0) == _lib.ERR_INVALID_IO_PATTERN
    assert call([0], n=0) == _lib.OK
    import poseidon252_amd as P
    with pytest.raises(P.InvalidIOPattern):
        gpu_ctx.hash_ragged(tags, flat, [0, 3, 3, 8], 1)
    with pytest.raises(ValueError):
        gpu_ctx.hash_ragged(tags, flat, [0, 5, 3, 8], 1)


def test_device_argument_checks(gpu_ctx):
    import torch
    from poseidon252_amd import _lib
    L = _lib.lib()
    t = torch.zeros((64, 4), dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda")
    s = ctypes_stream()
    p = t.data_ptr()
    assert L.p252_hash_ragged_device(gpu_ctx._h, p, 4, p + 8, off.data_ptr(), 1, p, 2, None, s) == _lib.ERR_INVALID_ARGUMENT  # misaligned
    assert L.p252_hash_ragged_device(gpu_ctx._h, p, 4, p, off.data_ptr(), 0, p, 2, None, s) == _lib.ERR_INVALID_IO_PATTERN
    assert L.p252_hash_ragged_device(gpu_ctx._h, None, 4, p, off.data_ptr(), 1, p, 2, None, s) == _lib.ERR_INVALID_ARGUMENT
    assert L.p252_hash_ragged_device(gpu_ctx._h, p, 0, p, off.data_ptr(), 1, p, 2, None, s) == _lib.ERR_INVALID_ARGUMENT
    assert L.p252_hash_ragged_device(gpu_ctx._h, None, 0, None, None, 1, None, 0, None, s) == _lib.OK
    torch.cuda.synchronize()


def ctypes_stream():
    import ctypes
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    """calls of different shapes on two streams of ONE context at the same time: each stream sorts in its own scratch"""
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import synth
    shapes = {"A": (300000, 42, 1), "B": (200000, 20, 3)}
    data = {}
    for k, (n, ml, ol) in shapes.items():
        lens = np.random.default_rng(n).integers(1, ml + 1, size=n).astype(np.uint64)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        d = synth.splitmix_scalars(n, int(off[-1]), "cuda:0")
        rb = P.RaggedHashBatch(P.Domain.Other, output_len=ol, ctx=gpu_ctx)
        ref = rb.digest((d, torch.from_numpy(off.view(np.int64)).cuda()), max_len=ml)  # alone, on the current stream
        data[k] = (rb, d, torch.from_numpy(off.view(np.int64)).cuda(), ml, ref, off)
    torch.cuda.synchronize()
    streams = {k: torch.cuda.Stream() for k in shapes}
    outs = {k: [] for k in shapes}
    for _ in range(3):
        for k in shapes:
            rb, d, d_off, ml, _, _ = data[k]
            with torch.cuda.stream(streams[k]):
                outs[k].append(rb.digest((d, d_off), max_len=ml))
    torch.cuda.synchronize()
    for k in shapes:
        rb, d, d_off, ml, ref, off = data[k]
        for o in outs[k]:
            assert torch.equal(o, ref), k
        rows = np.arange(0, shapes[k][0], 331)
        exp = _oracle(oracle_mod, d.cpu().numpy().view(np.uint64), off, shapes[k][2], rows)
        assert np.array_equal(ref.cpu().numpy().view(np.uint64)[rows], exp), k


def test_input_beyond_4_gib(gpu_ctx, oracle_mod):
    """>= 2^27 scalars in one array: scalar offsets past 2^27, byte offsets past 2^32; sampled messages against the oracle"""
    import torch
    import poseidon252_amd as P
    total = (1 << 27) + 4096
    rng = np.random.default_rng(27)
    lens = rng.integers(900, 1001, size=total // 900 + 1).astype(np.uint64)
    off = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    n = int(np.searchsorted(off, total))
    off = off[:n + 1]
    S = int(off[-1])
    assert S >= 1 << 27 and S * 32 > 1 << 32
    d = torch.randint(-(1 << 62), 1 << 62, (S, 4), dtype=torch.int64, device="cuda")
    d[:, 3] &= 0x0FFFFFFFFFFFFFFF  # < 2^252 < p: fully reduced scalars
    rb = P.RaggedHashBatch(P.Domain.Other, ctx=gpu_ctx)
    got = rb.digest((d, torch.from_numpy(off.view(np.int64)).cuda()), max_len=1000).cpu().numpy().view(np.uint64)
    rows = np.unique(np.concatenate([np.arange(0, n, n // 12), np.arange(n - 4, n)]))
    assert int(off[rows[-1]]) * 32 > 1 << 32
    sub_off = np.zeros(rows.size + 1, np.uint64)
    parts = []
    for i, r in enumerate(rows):
        part = d[int(off[r]):int(off[r + 1])].cpu().numpy().view(np.uint64)
        parts.append(part)
        sub_off[i + 1] = sub_off[i] + part.shape[0]
    exp = _oracle(oracle_mod, np.concatenate(parts), sub_off, 1)
    assert np.array_equal(got[rows], exp)
    del d
    torch.cuda.empty_cache()


# floors from profiles/r07_ragged.txt: sorted / unsorted measured 1.93 (floor 1.6: -17 %); the ragged call's useful permutation rate
# measured 0.99 of the uniform 42 -> 1 batch's (floor 0.90: -9 %, both run the same sponge body under the same power cap)
SORTED_OVER_UNSORTED_FLOOR = 1.6
RATE_OVER_UNIFORM_FLOOR = 0.90


def test_sorted_schedule_pays(gpu_ctx):
    """2^20 messages, lengths uniform in 1..42, out_len 1 (bench_tools/ragged_bench.py): the sorted call against the same call under
    P252_RAGGED_SORT=0, and its useful permutation rate against the uniform 42 -> 1 batch"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "ragged_bench.py"), "--reps", "20", "--skip", "d"], cwd=ROOT,
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["outputs_equal"]["a_b"]
    assert res["sorted_over_unsorted"] >= SORTED_OVER_UNSORTED_FLOOR, res
    assert res["ragged_rate_over_uniform"] >= RATE_OVER_UNIFORM_FLOOR, res


def test_cpp_mirror_on_gpu(tmp_path, oracle_mod, gpu_ctx):
    assert "ALL PASSED" in run_cpp_mirror(build_cpp_mirror("test_ragged_api", tmp_path, flags=()))
