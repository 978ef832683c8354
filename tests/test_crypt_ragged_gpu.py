"""Messages of different lengths encrypted and decrypted in one call (p252_{encrypt,decrypt}_ragged*, csrc/crypt_ragged.hip and the
RAGGED instantiations of k_crypt / k_crypt_coop) on the GPU, checked against the oracle's encrypt run per length and against the
fixed-length call.  Batches of at most 8,192 messages take the lane-group build, larger ones the one-lane build;
P252_COOP_MAX_NODES=0 (read once per process: a child) gives the one-lane build on a small batch."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import cryptragged as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = list(range(1, 19)) + [21, 41, 42, 43]
FILL = 0x5A5A5A5A5A5A5A5A
VARIANTS = (0, 1)  # P252_CRYPT_STREAM, P252_CRYPT_DUPLEX


_shuffled, _round_trip = CR.shuffled, CR.round_trip


_ONE_LANE_CHILD = """
import sys
sys.path.insert(0, %r)
import oracle, poseidon252_amd as P
from testsupport import cryptragged as CR
oracle.build()
for variant in (0, 1):
    CR.round_trip(P.Context(0), oracle, variant, CR.shuffled(variant, %r), 70 + variant, 43)
print("one-lane ok")
"""


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_length_matches_the_oracle(gpu_ctx, oracle_mod, variant):
    """lengths 1..18, 21, 41, 42, 43 in shuffled order on the lane-group build, then the same messages repeated past 8,192 (the
    one-lane build) with the expected rows broadcast"""
    lens = _shuffled(variant, LENS)
    (flat, off, sec, non), want = _round_trip(gpu_ctx, oracle_mod, variant, lens, 70 + variant, 43)
    reps = 8200 // len(lens) + 1
    big_off = CR.offsets_of(lens * reps)
    big = (np.concatenate([flat] * reps), big_off, np.concatenate([sec] * reps), np.concatenate([non] * reps))
    got = CR.device_encrypt(gpu_ctx, *big, variant, 43)
    assert np.array_equal(got.reshape(reps, -1, 4), np.broadcast_to(want, (reps,) + want.shape))
    back, ok = CR.device_decrypt(gpu_ctx, got, big_off, big[2], big[3], variant, 43, big[0].shape[0])
    assert np.array_equal(back, big[0]) and (ok == 1).all()


def test_every_length_on_the_one_lane_build_of_a_small_batch():
    code = _ONE_LANE_CHILD % (ROOT, LENS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, P252_COOP_MAX_NODES="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "one-lane ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _equals_the_fixed_call(ctx, oracle_mod, counts, seed, variant=0):
    """every ciphertext of the ragged call is byte-equal to p252_encrypt_batch_device on the gathered messages of its length"""
    import torch
    from poseidon252_amd import encryption as E
    lens = _shuffled(seed, [L for L, c in counts.items() for _ in range(c)])
    flat, off, sec, non = CR.case(oracle_mod, seed, lens)
    got = CR.device_encrypt(ctx, flat, off, sec, non, variant, max(counts))
    lens = np.asarray(lens)
    for L in counts:
        ids = np.nonzero(lens == L)[0]
        x = np.stack([flat[int(off[i]):int(off[i + 1])] for i in ids])
        d_c = torch.zeros((ids.size, L + 1, 4), dtype=torch.int64, device="cuda")
        E.encrypt_batch_device(CR.to_dev(x), CR.to_dev(sec[ids]), CR.to_dev(non[ids]), L, d_c, ids.size, ctx=ctx, variant=variant)
        fixed = d_c.cpu().numpy().view(np.uint64)
        assert np.array_equal(np.stack([got[CR.cipher_rows(off, i)] for i in ids]), fixed), L


def test_schedule_edges_equal_the_fixed_length_call(gpu_ctx, oracle_mod):
    # 63, 64 and 65 messages of three lengths beside one lone message of length 42, above 8,192 in all: the one-lane build (G = 64)
    _equals_the_fixed_call(gpu_ctx, oracle_mod, {3: 63, 5: 64, 9: 65, 42: 1, 2: 8100}, 11)
    # 7, 8 and 9 messages on the lane-group build (G = 8)
    _equals_the_fixed_call(gpu_ctx, oracle_mod, {3: 7, 5: 8, 9: 9, 42: 1}, 12, variant=1)
    _equals_the_fixed_call(gpu_ctx, oracle_mod, {6: 1}, 13)  # n = 1


def test_the_cap(gpu_ctx, oracle_mod):
    """three messages of lengths 2,048, 2,047 and 1 against the oracle; max_len = 2,049 is refused"""
    import torch
    from poseidon252_amd import _lib
    for variant in VARIANTS:
        _round_trip(gpu_ctx, oracle_mod, variant, [CR.CAP, CR.CAP - 1, 1], 30 + variant, CR.CAP)
    t = torch.zeros((CR.CAP + 8, 4), dtype=torch.int64, device="cuda")
    off = CR.to_dev(CR.offsets_of([1]))
    rc = _lib.lib().p252_encrypt_ragged_device_into(gpu_ctx._h, 0, t.data_ptr(), CR.CAP + 1, t.data_ptr() + 64, 1, off.data_ptr(), t.data_ptr() + 128,
                                               t.data_ptr() + 256, t.data_ptr() + 512, 1, None, None)
    assert rc == _lib.ERR_INVALID_ARGUMENT and str(CR.CAP) in _lib.lib().p252_last_error(gpu_ctx._h).decode()
    with pytest.raises(Exception):
        from poseidon252_amd import encryption as E
        E.encryption_tags(CR.CAP + 1)


@pytest.mark.parametrize("n_valid_pad", [0, 9000])
def test_bad_messages(gpu_ctx, oracle_mod, n_valid_pad):
    """an empty message, one above max_len, a decreasing pair and an end past n_scalars: d_n_bad exact, their pre-filled output regions
    untouched, ok = 0 on decrypt, every valid message exact (with 9,000 valid messages beside them the one-lane build runs)"""
    import torch
    max_len = 42
    lens = [5, 0, 42, 43, 7, 3, 1, 3] + [int(x) for x in np.random.default_rng(3).integers(1, 43, size=n_valid_pad)] + [4]
    flat, off, sec, non = CR.case(oracle_mod, 91, lens)
    off[5] = off[4] - 2  # message 4 becomes a decreasing pair; message 5 grows to 2 + 7 + 3 = 12 scalars and stays valid
    n, n_scalars = len(lens), flat.shape[0] - 1  # the last message ends one scalar past n_scalars
    bad = CR.bad_messages(off, max_len, n_scalars)
    assert list(np.nonzero(bad)[0]) == [1, 3, 4, n - 1]
    valid = np.nonzero(~bad)[0]
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = CR.device_encrypt(gpu_ctx, flat, off, sec, non, 0, max_len, prefill=FILL, d_bad=d_bad, n_scalars=n_scalars)
    assert int(d_bad.item()) == int(bad.sum())
    ref = CR.oracle_ciphers(oracle_mod, flat, off, sec, non, 0, rows=valid)
    want = np.full((n_scalars + n, 4), FILL, dtype=np.uint64)
    for i in valid:  # (no two VALID messages overlap here: everything else keeps the fill)
        want[CR.cipher_rows(off, i)] = ref[CR.cipher_rows(off, i)]
    assert np.array_equal(got, want)
    d_bad.zero_()
    back, ok = CR.device_decrypt(gpu_ctx, got, off, sec, non, 0, max_len, n_scalars, prefill=FILL, d_bad=d_bad)
    assert int(d_bad.item()) == int(bad.sum())
    assert np.array_equal(ok, (~bad).astype(np.uint8))
    want_m = np.full((n_scalars, 4), FILL, dtype=np.uint64)
    for i in valid:
        want_m[int(off[i]):int(off[i + 1])] = flat[int(off[i]):int(off[i + 1])]
    assert np.array_equal(back, want_m)


def test_tampering_fails_exactly_the_tampered_messages(gpu_ctx, oracle_mod):
    lens = _shuffled(5, LENS)
    for variant in VARIANTS:
        (flat, off, sec, non), c = _round_trip(gpu_ctx, oracle_mod, variant, lens, 50 + variant, 43)
        c, sec, non = c.copy(), sec.copy(), non.copy()
        c[int(off[2]) + 2, 0] ^= np.uint64(1)  # the first cipher scalar of message 2
        c[CR.cipher_rows(off, 7).stop - 1, 1] ^= np.uint64(4)  # the MAC of message 7
        sec[11, 1, 2] ^= np.uint64(1 << 40)
        non[17, 0] += np.uint64(1)
        _, ok = CR.device_decrypt(gpu_ctx, c, off, sec, non, variant, 43, flat.shape[0])
        want = np.ones(len(lens), dtype=np.uint8)
        want[[2, 7, 11, 17]] = 0
        assert np.array_equal(ok, want), variant


@pytest.mark.parametrize("n", [64, 8256])
def test_edge_values_through_both_new_instantiations(gpu_ctx, oracle_mod, n):
    """messages, secrets and nonces of 0, 1, p - 1, non-canonical limbs up to 2^256 - 1 and saturated digits (the generators of
    tests/edgecases.py) against the oracle on the values mod p: n = 64 the lane-group build, 8,256 the one-lane build.  Decrypt
    compares the MAC as stored bytes: MAC + p fails, an unreduced cipher ELEMENT does not."""
    import edgecases as EC
    lens = _shuffled(n, ([1, 4, 5, 9, 2, 7, 21, 3] * (n // 8)))
    off = CR.offsets_of(lens)
    S = int(off[-1])
    for variant in VARIANTS:
        raw, red = EC.edge_scalars(0x6100 + n + variant, S + 3 * n)
        parts = lambda a: (a[:S], a[S:S + 2 * n].reshape(n, 2, 4), a[S + 2 * n:])
        got = CR.device_encrypt(gpu_ctx, *parts(raw)[:1], off, *parts(raw)[1:], variant, 21)
        m_red, s_red, n_red = parts(red)
        assert EC.is_reduced(got).all()
        assert np.array_equal(got, CR.oracle_ciphers(oracle_mod, m_red, off, s_red, n_red, variant))
        twin = got.copy()
        for i in range(n):  # every message element of every cipher as its unreduced twin, the MACs as stored
            rows = CR.cipher_rows(off, i)
            twin[rows.start:rows.stop - 1] = EC.unreduced_twin(got[rows.start:rows.stop - 1])
        mac_rows = [CR.cipher_rows(off, i).stop - 1 for i in (0, n // 2, n - 1)]
        twin[mac_rows] = EC.plus_p(got[mac_rows])  # the same residue, other bytes: refused
        back, ok = CR.device_decrypt(gpu_ctx, twin, off, parts(raw)[1], parts(raw)[2], variant, 21, S)
        want_ok = np.ones(n, dtype=np.uint8)
        want_ok[[0, n // 2, n - 1]] = 0
        assert np.array_equal(ok, want_ok)
        assert np.array_equal(back, m_red)  # (the message does not depend on the MAC)


def _device_case(oracle_mod, seed, n, max_len):
    import torch
    lens = np.random.default_rng(seed).integers(1, max_len + 1, size=n)
    flat, off, sec, non = CR.case(oracle_mod, seed, lens)
    return [CR.to_dev(x) for x in (flat, off, sec, non)] + [torch.zeros((flat.shape[0] + n, 4), dtype=torch.int64, device="cuda"), n, max_len]


def test_two_streams_of_one_context_and_a_graph(gpu_ctx, oracle_mod):
    """calls of different shapes on two streams of ONE context at the same time (each stream schedules in its own scratch), and one
    linear single-stream graph capture replayed twice: the bytes of the call run alone"""
    import torch
    from poseidon252_amd import encryption as E
    cases = {"A": _device_case(oracle_mod, 1, 20000, 42), "B": _device_case(oracle_mod, 2, 3000, 20)}
    ref = {}
    for k, (m, o, s, nn, c, n, ml) in cases.items():
        E.encrypt_ragged_device(m, o, s, nn, c, n, ml, ctx=gpu_ctx)
        ref[k] = c.clone()
    torch.cuda.synchronize()
    streams = {k: torch.cuda.Stream() for k in cases}
    outs = {k: [] for k in cases}
    for _ in range(3):
        for k, (m, o, s, nn, c, n, ml) in cases.items():
            with torch.cuda.stream(streams[k]):
                out = torch.zeros_like(c)
                E.encrypt_ragged_device(m, o, s, nn, out, n, ml, ctx=gpu_ctx)
                outs[k].append(out)
    torch.cuda.synchronize()
    for k in cases:
        assert all(torch.equal(o, ref[k]) for o in outs[k]), k
    m, o, s, nn, c, n, ml = cases["B"]
    flat, off = m.cpu().numpy().view(np.uint64), o.cpu().numpy().view(np.uint64)
    rows = np.arange(0, n, 97)
    want = CR.oracle_ciphers(oracle_mod, flat, off, s.cpu().numpy().view(np.uint64).reshape(n, 2, 4), nn.cpu().numpy().view(np.uint64), 0, rows=rows)
    got = ref["B"].cpu().numpy().view(np.uint64)
    for i in rows:
        assert np.array_equal(got[CR.cipher_rows(off, i)], want[CR.cipher_rows(off, i)]), i
    side = torch.cuda.Stream()
    out = torch.zeros_like(c)
    with torch.cuda.stream(side):
        E.encrypt_ragged_device(m, o, s, nn, out, n, ml, ctx=gpu_ctx)  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        E.encrypt_ragged_device(m, o, s, nn, out, n, ml, ctx=gpu_ctx)
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref["B"])


def test_host_twins(gpu_ctx, oracle_mod):
    """they equal the device path; the error codes are hash_ragged's; nothing of the call is left in library-owned memory"""
    import poseidon252_amd as P
    from poseidon252_amd import _lib, encryption as E
    L = _lib.lib()
    ctx = P.Context(0)  # a context that has done nothing else
    lens = _shuffled(9, LENS)
    flat, off, sec, non = CR.case(oracle_mod, 9, lens)
    msgs = [flat[int(off[i]):int(off[i + 1])] for i in range(len(lens))]
    for variant in VARIANTS:
        dev = CR.device_encrypt(gpu_ctx, flat, off, sec, non, variant, 43)
        c_flat, c_off = E.encrypt_ragged((flat, off), sec, non, ctx=ctx, variant=variant)
        assert np.array_equal(c_flat, dev) and np.array_equal(c_off, off)
        c_list = E.encrypt_ragged(msgs, sec, non, ctx=ctx, variant=variant)
        assert all(np.array_equal(c, dev[CR.cipher_rows(off, i)]) for i, c in enumerate(c_list))
        (back, _), ok = E.decrypt_ragged((c_flat, off), sec, non, ctx=ctx, variant=variant)
        assert np.array_equal(back, flat) and ok.all()
        assert all(np.array_equal(a, b) for a, b in zip(E.decrypt_ragged_checked(c_list, sec, non, ctx=ctx, variant=variant), msgs))
        c_list[3] = c_list[3].copy()
        c_list[3][-1, 0] ^= np.uint64(1)
        _, ok = E.decrypt_ragged(c_list, sec, non, ctx=ctx, variant=variant)
        assert list(np.nonzero(~ok)[0]) == [3]
        with pytest.raises(E.DecryptionFailed, match="message 3"):
            E.decrypt_ragged_checked(c_list, sec, non, ctx=ctx, variant=variant)
    residue = ctypes.c_uint64(1)
    assert L.p252_scratch_residue(ctx._h, ctypes.byref(residue)) == 0 and residue.value == 0
    u64p = ctypes.POINTER(ctypes.c_uint64)
    tags = E.encryption_tags(8)
    out = np.zeros((32, 4), np.uint64)

    def call(offsets, max_len=8, n=None):
        o = np.asarray(offsets, np.uint64)
        return L.p252_encrypt_ragged(ctx._h, 0, tags.ctypes.data_as(u64p), max_len, flat.ctypes.data_as(u64p), o.ctypes.data_as(u64p),
                                     sec.ctypes.data_as(u64p), non.ctypes.data_as(u64p), out.ctypes.data_as(u64p), o.size - 1 if n is None else n)
    assert call([0, 3, 5, 8]) == _lib.OK
    assert call([0, 3, 3, 8]) == _lib.ERR_INVALID_IO_PATTERN and "message 1 is empty" in L.p252_last_error(ctx._h).decode()
    assert call([0, 5, 3, 8]) == _lib.ERR_INVALID_ARGUMENT and "decrease at message 1" in L.p252_last_error(ctx._h).decode()
    assert call([0, 3, 12, 14]) == _lib.ERR_INVALID_ARGUMENT and "message 1 is longer than max_len" in L.p252_last_error(ctx._h).decode()
    assert call([0, 3], max_len=CR.CAP + 1) == _lib.ERR_INVALID_ARGUMENT and str(CR.CAP) in L.p252_last_error(ctx._h).decode()
    assert call([0], n=0) == _lib.OK
    with pytest.raises(P.InvalidIOPattern):
        E.encrypt_ragged((flat, [0, 3, 3, 8]), sec[:3], non[:3], ctx=ctx)
    with pytest.raises(ValueError):
        E.encrypt_ragged((flat, [0, 5, 3, 8]), sec[:3], non[:3], ctx=ctx)
    assert L.p252_scratch_residue(ctx._h, ctypes.byref(residue)) == 0 and residue.value == 0


def test_cpp_mirror_on_gpu(tmp_path, oracle_mod, gpu_ctx):
    assert "ALL PASSED" in run_cpp_mirror(build_cpp_mirror("test_crypt_ragged_api", tmp_path, flags=()))


# floors from profiles/crypt_ragged.txt (bench_tools/crypt_ragged_bench.py, medians of 20 in one run): the measured ratio less 10 % at
# equal lengths (box-to-box clock spread under the power cap, the allowance of test_ragged_gpu.py), less 15 % against the
# per-length loop.  Measured at 2.40-2.42 GHz: ragged over fixed 0.9956 (floor 0.896), ragged over the loop 3.3487 (floor 2.846)
RAGGED_OVER_FIXED_FLOOR = 0.896
RAGGED_OVER_LOOP_FLOOR = 2.846


def test_rate(gpu_ctx):
    """2^20 messages: the ragged call against p252_encrypt_batch_device at equal lengths (42), and against one gather plus one
    fixed-length call per distinct length at lengths uniform in 1..42"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "crypt_ragged_bench.py"), "--reps", "20", "--no-profile"], cwd=ROOT,
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["outputs_equal"]
    assert res["ragged_over_fixed_equal_lengths"] >= RAGGED_OVER_FIXED_FLOOR, res
    assert res["ragged_over_per_length_loop"] >= RAGGED_OVER_LOOP_FLOOR, res
