"""Messages of different lengths encrypted and decrypted in one call (p252_{encrypt,decrypt}_ragged*), the parts that need no GPU:
the tag table, the ABI, the argument refusals, a numpy model of the schedule, the call sequence the kernels compute, what hipcc
generates for the new instantiations, and the Python and C++ mirrors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import shapecases
from helpers.binding import _dev, _no_device_context, recorder, with_cpu_tensor  # noqa: F401  (recorder: a fixture)
from helpers.percall import CPP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table
from testsupport import cryptragged as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = ctypes.POINTER(ctypes.c_uint64)


# ---------------------------------------------------------------------------------------------- the tag table
@pytest.mark.parametrize("variant", [0, 1])
def test_tag_table_equals_the_tag_row_by_row(variant):
    from poseidon252_amd import _lib
    L = _lib.lib()
    for max_len in (1, 42, CR.CAP):
        tags = np.zeros((max_len, 4), dtype=np.uint64)
        assert L.p252_encryption_tags(variant, max_len, tags.ctypes.data_as(U64P)) == _lib.OK
        one = np.zeros(4, dtype=np.uint64)
        for length in range(1, max_len + 1):
            assert L.p252_encryption_tag(variant, length, one.ctypes.data_as(U64P)) == _lib.OK
            assert np.array_equal(tags[length - 1], one), (max_len, length)
    spare = np.zeros((CR.CAP + 1, 4), dtype=np.uint64)
    for max_len in (0, CR.CAP + 1):
        assert L.p252_encryption_tags(variant, max_len, spare.ctypes.data_as(U64P)) == _lib.ERR_INVALID_ARGUMENT
    assert not spare.any()
    assert L.p252_encryption_tags(2, 4, spare.ctypes.data_as(U64P)) == _lib.ERR_INVALID_ARGUMENT
    assert L.p252_encryption_tags(variant, 4, None) == _lib.ERR_INVALID_ARGUMENT


def test_python_tag_table():
    import poseidon252_amd as P
    from poseidon252_amd import encryption as E
    t = P.encryption_tags(42, E.DUPLEX)
    assert t.shape == (42, 4) and np.array_equal(t[20], P.encryption_tag(21, E.DUPLEX)) and not np.array_equal(t[20], P.encryption_tags(42)[20])
    assert E.RAGGED_MAX_LEN == CR.CAP
    for bad in (0, CR.CAP + 1):
        with pytest.raises(ValueError):
            P.encryption_tags(bad)


# ---------------------------------------------------------------------------------------------- the ABI
def test_abi_symbols_and_documents():
    raw, _ = check_abi_symbols(CR.SYMBOLS)
    assert re.search(r"#define P252_CRYPT_RAGGED_MAX_LEN %d\b" % CR.CAP, raw)
    version_comment = raw[raw.index("   9  + p252_hash_ragged"):raw.index("#define P252_ABI_VERSION")]
    assert "p252_encryption_tags, p252_{encrypt,decrypt}_ragged[_device_into] (additive, same version)" in version_comment
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration and "p252_encrypt_ragged" in integration
    for doc in ("README.md", "DESIGN.md"):
        assert "p252_{encrypt,decrypt}_ragged" in open(os.path.join(ROOT, doc)).read(), doc


def test_refusal_table(tmp_path):
    table = refusal_table("crypt_ragged_refusal_table", tmp_path)
    assert_rows_equal_golden(table, "crypt_ragged_refusals")
    by = {(r[0], r[1]): r for r in table}
    for sym in ("p252_encrypt_ragged_device_into", "p252_decrypt_ragged_device_into"):
        assert by[(sym, "control")][2] == -4 and by[(sym, "variant=DUPLEX")][2] == -4  # past validation: P252_ERR_HIP at the device
        assert by[(sym, "n=0")][2] == 0 and by[(sym, "n=0,all=NULL")][2] == 0
        for case in ("max_len=0", "max_len=cap+1", "max_len=SIZE_MAX"):
            assert by[(sym, case)][2] == -3 and "P252_CRYPT_RAGGED_MAX_LEN = %d" % CR.CAP in by[(sym, case)][3], case
        assert by[(sym, "max_len=cap")][2] == -4 and by[(sym, "d_n_bad=NULL")][2] == -4
        assert by[(sym, "d_out=d_in")][2] == -3 and "overlaps" in by[(sym, "d_out=d_in")][3]
        assert by[(sym, "n_scalars+n=SIZE_MAX/64")][2] == -3 and "overflow" in by[(sym, "n_scalars+n=SIZE_MAX/64")][3]
        for (s, case), r in by.items():
            if s == sym and (case.endswith("=NULL") and case != "d_n_bad=NULL" and case != "n=0,all=NULL" or "+last" in case or re.search(r"\+\d+$", case)):
                assert r[2] == -3, (sym, case)
            if s == sym and case.endswith("+end"):
                assert r[2] == -4, (sym, case)  # just behind the other buffer: no overlap


# ---------------------------------------------------------------------------------------------- the schedule
def _check_schedule(off, max_len, n_scalars, coop):
    n, g = off.size - 1, CR.group(coop)
    order, bucket = CR.schedule(off, max_len, n_scalars, coop)
    assert order.size == CR.slot_bound(n, max_len, coop) and order.size % g == 0  # the launched bound holds (schedule asserts it too)
    live = order[order != CR.SENTINEL]
    assert np.array_equal(np.sort(live), np.arange(n, dtype=np.uint64))  # every message once
    seen = []
    for s in range(0, order.size, g):
        ids = order[s:s + g]
        ids = ids[ids != CR.SENTINEL]
        if ids.size:
            b = set(bucket[ids.astype(np.int64)].tolist())
            assert len(b) == 1, (s, b)  # one length per group, or sentinels
            seen.append(b.pop())
    keys = [max_len + 1 if b == 0 else max_len - b for b in seen]  # descending lengths, the bad messages (bucket 0) last
    assert keys == sorted(keys)
    return order


@pytest.mark.parametrize("coop", [True, False])
def test_schedule_model(coop):
    g = CR.group(coop)
    _check_schedule(CR.offsets_of([5]), 42, 5, coop)  # n = 1
    for count in (g - 1, g, g + 1):
        lens = [3] * count + [9] * count + [42]
        np.random.default_rng(count).shuffle(lens)
        off = CR.offsets_of(lens)
        order = _check_schedule(off, 42, int(off[-1]), coop)
        assert np.count_nonzero(order != CR.SENTINEL) == 2 * count + 1
    lens = list(range(1, 65))  # all max_len lengths distinct: the padding at its worst, still inside the bound
    off = CR.offsets_of(lens)
    order = _check_schedule(off, 64, int(off[-1]), coop)
    assert np.flatnonzero(order != CR.SENTINEL)[-1] == 63 * g
    bad = CR.offsets_of([0, 50, 0, 43])  # all bad: empty, above max_len
    order = _check_schedule(bad, 42, int(bad[-1]), coop)
    assert set(order[:4].tolist()) == {0, 1, 2, 3}
    off = CR.offsets_of([5, 7, 3])
    off[2] = off[1] - 2  # a decreasing pair, and the last message past n_scalars
    assert list(CR.bad_messages(off, 42, int(off[-1]) - 1)) == [False, True, True]
    _check_schedule(off, 42, int(off[-1]) - 1, coop)
    for n, ml in ((1, 1), (8192, CR.CAP), (8193, CR.CAP), (1 << 20, 42)):  # the bound as csrc/crypt_ragged.h states it
        assert CR.slot_bound(n, ml, coop) == -(-(n + (g - 1) * (ml + 1)) // g) * g


def test_schedule_source_states_the_model():
    csrc = os.path.join(ROOT, "poseidon252_amd", "csrc")
    h = open(os.path.join(csrc, "crypt_ragged.h")).read()
    assert "return coop ? 8 : 64;" in h and "(n + (g - 1) * (max_len + 1) + g - 1) / g * g" in h
    assert "CRYPT_RAGGED_BUCKETS = P252_CRYPT_RAGGED_MAX_LEN + 1" in h
    assert "return b <= a || b - a > max_len || b > n_scalars;" in open(os.path.join(csrc, "crypt_args.h")).read()


# ---------------------------------------------------------------------------------------------- the call sequence of the kernels
def test_generated_call_sequence_equals_the_call_table(tmp_path):
    exe = str(tmp_path / "crypt_calls_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(CPP, "crypt_calls_dump.cpp"), "-o", exe])
    lengths = list(range(1, 65)) + [CR.CAP]
    out = subprocess.run([exe] + [str(x) for x in lengths], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 2 * len(lengths)
    for line in out:
        variant, length, calls = line.split("\t")
        got = [tuple(int(x) for x in c.split(":")) for c in calls.split(" ")]
        assert got == shapecases.crypt_program(int(variant), int(length)), (variant, length)
    src = open(os.path.join(ROOT, "poseidon252_amd", "csrc", "kernels.hip")).read()
    assert '#include "crypt_calls.hpp"' in src and src.count("crypt_call(variant, len, ci)") == 2  # the kernels call this very header


# ---------------------------------------------------------------------------------------------- what hipcc generates
@pytest.fixture(scope="module")
def kernels_isa():
    """(ISA text, resource-usage remarks) of kernels.hip: the compile tests/test_kernel_resources.py and tests/test_isa_counts.py share"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_count as ic
    out, remarks = ic.compile_asm(with_remarks=True)
    return open(out).read(), remarks


def test_new_instantiations_meet_the_register_conditions(kernels_isa):
    _, remarks = kernels_isa
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", remarks)]
    agprs = [int(x) for x in re.findall(r"\bAGPRs: (\d+)", remarks)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks)]
    rows = {n: (s, v, a, o) for n, s, v, a, o in zip(names, scratch, vgprs, agprs, occ)}
    ragged = sorted(n for n in rows if re.search(r"k_crypt(_coop)?ILb[01]ELb1EE", n))
    fixed = sorted(n for n in rows if re.search(r"k_crypt(_coop)?ILb[01]ELb0EE", n))
    assert len(ragged) == 4 and len(fixed) == 4, names
    for n in ragged:
        s, v, a, o = rows[n]
        assert s == 0 and a == 0 and v <= 256 and (o >= 2 or "_coop" in n) and ("_coop" in n or v < 256), (n, rows[n])


def test_schedule_kernels_do_not_hash_and_use_no_private_memory(tmp_path):
    """the four kernels of the schedule live beside the counting sort they are modelled on (csrc/ragged.hip: the files that may call the
    bucket primitives are a fixed set); crypt_ragged.hip is the launcher and holds no kernel"""
    import edgecases
    from helpers.kernel_resources import kernel_resources
    res, text = kernel_resources("ragged.hip", tmp_path / "ragged.s")
    mine = {n: v for n, v in res.items() if "k_crypt_ragged_" in n}
    assert len(mine) == 4, list(res)
    assert all(v["scratch"] == 0 and v["vgpr"] <= 64 for v in mine.values()), mine
    for n in mine:
        body = text[text.index("\n" + n + ":"):]
        assert "scratch_" not in body[:body.index("s_endpgm")], n
    csrc = os.path.join(ROOT, "poseidon252_amd", "csrc")
    launcher = open(os.path.join(csrc, "crypt_ragged.hip")).read()
    assert "__global__" not in launcher and "hades_permute" not in launcher and "hades29.hpp" not in launcher
    funcs = {name: body for _, name, body in edgecases._functions(open(os.path.join(csrc, "ragged.hip")).read())}
    for k in ("k_crypt_ragged_clear", "k_crypt_ragged_hist", "k_crypt_ragged_scan", "k_crypt_ragged_scatter"):
        assert "hades_permute" not in funcs[k] and "node_digest" not in funcs[k], k
    # no hashing kernel has a name the edge-value matrix does not know: the mixed-length mode is an instantiation of k_crypt / k_crypt_coop
    assert edgecases.hashing_kernels() <= edgecases.named_kernels()
    assert not any("crypt_ragged" in k for k in edgecases.hashing_kernels())


# ---------------------------------------------------------------------------------------------- the Python mirror
def _device_args(decrypt, n=6, n_scalars=100, max_len=42):
    a = {"d_tags": _dev(max_len * 4), ("d_ciphers" if decrypt else "d_messages"): _dev((n_scalars + (n if decrypt else 0)) * 4),
         "d_offsets": _dev(n + 1), "d_secrets": _dev(n * 8), "d_nonces": _dev(n * 4),
         ("d_messages" if decrypt else "d_ciphers"): _dev((n_scalars + (0 if decrypt else n)) * 4)}
    if decrypt:
        a["d_ok"] = _dev(n, torch.uint8)
    a["d_n_bad"] = _dev(1, torch.int32)
    return a


def _call(ctx, decrypt, a, n=6, n_scalars=100, max_len=42):
    if decrypt:
        ctx.decrypt_ragged_device(0, a["d_tags"], max_len, a["d_ciphers"], n_scalars, a["d_offsets"], a["d_secrets"], a["d_nonces"], a["d_messages"],
                                  a["d_ok"], n, d_n_bad=a["d_n_bad"])
    else:
        ctx.encrypt_ragged_device(0, a["d_tags"], max_len, a["d_messages"], n_scalars, a["d_offsets"], a["d_secrets"], a["d_nonces"], a["d_ciphers"], n,
                                  d_n_bad=a["d_n_bad"])


@pytest.mark.parametrize("decrypt", [False, True])
def test_python_methods_check_their_tensors_before_the_library(recorder, decrypt):  # noqa: F811
    ctx = _no_device_context()
    name = "p252_decrypt_ragged_device_into" if decrypt else "p252_encrypt_ragged_device_into"
    good = _device_args(decrypt)
    _call(ctx, decrypt, good)
    assert recorder.calls == [name]
    _call(ctx, decrypt, dict(good, d_n_bad=None))  # optional
    assert recorder.calls == [name] * 2
    for arg, args in with_cpu_tensor(good):
        with pytest.raises(ValueError, match=arg):
            _call(ctx, decrypt, args)
    # one element short of what the call touches; the cipher side holds n_scalars + n scalars
    sizes = {"d_tags": 42 * 4, "d_offsets": 7, "d_secrets": 48, "d_nonces": 24, "d_messages": 400, "d_ciphers": 424, "d_ok": 6, "d_n_bad": 1}
    for arg, t in good.items():
        short = _dev(sizes[arg] - 1, t.dtype)
        with pytest.raises(ValueError, match=arg):
            _call(ctx, decrypt, dict(good, **{arg: short}))
    with pytest.raises(ValueError, match="d_offsets"):
        _call(ctx, decrypt, dict(good, d_offsets=_dev(14, torch.int32)))  # 4-byte elements
    assert recorder.calls == [name] * 2  # nothing else reached the library


def test_python_passes_the_sizes(monkeypatch):
    from poseidon252_amd import _lib
    seen = []

    class Spy:
        def __getattr__(self, name):
            def call(*args):
                seen.append((name, args))
                return 0
            return call
    monkeypatch.setattr(_lib, "_lib", Spy())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0})())
    ctx = _no_device_context()
    for decrypt in (False, True):
        _call(ctx, decrypt, _device_args(decrypt))
    (n0, a0), (n1, a1) = seen
    assert n0 == "p252_encrypt_ragged_device_into" and (a0[1], a0[3], a0[5], a0[10]) == (0, 42, 100, 6) and len(a0) == 13
    assert n1 == "p252_decrypt_ragged_device_into" and (a1[1], a1[3], a1[5], a1[11]) == (0, 42, 100, 6) and len(a1) == 14


def test_helpers_are_exported_and_check_their_lists():
    import poseidon252_amd as P
    from poseidon252_amd import encryption as E
    names = {"encryption_tags", "encrypt_ragged", "decrypt_ragged", "decrypt_ragged_checked", "encrypt_ragged_device", "decrypt_ragged_device"}
    assert names <= set(P.__all__) and all(getattr(P, n) is getattr(E, n) for n in names)
    m = [np.ones((3, 4), np.uint64), np.zeros((0, 4), np.uint64)]
    with pytest.raises(P.InvalidIOPattern, match="message 1 is empty"):
        P.encrypt_ragged(m, np.zeros((2, 2, 4), np.uint64), np.zeros((2, 4), np.uint64))
    with pytest.raises(ValueError, match="decrease at message 1"):
        P.encrypt_ragged((np.ones((8, 4), np.uint64), [0, 5, 3, 8]), np.zeros((3, 2, 4), np.uint64), np.zeros((3, 4), np.uint64))
    with pytest.raises(ValueError, match="longer than max_len"):
        P.encrypt_ragged([np.ones((9, 4), np.uint64)], np.zeros((1, 2, 4), np.uint64), np.zeros((1, 4), np.uint64), max_len=8)
    with pytest.raises(P.InvalidIOPattern, match="message 0 is empty"):
        P.decrypt_ragged([np.ones((1, 4), np.uint64)], np.zeros((1, 2, 4), np.uint64), np.zeros((1, 4), np.uint64))
    assert P.encrypt_ragged([], np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64)) == []


# ---------------------------------------------------------------------------------------------- the C++ mirror and the bench tool
def test_cpp_mirror_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_crypt_ragged_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("crypt_ragged_bench", ("--quick", "--reps"))
