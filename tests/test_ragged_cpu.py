"""Messages of different lengths in one call (p252_hash_ragged*, csrc/ragged.hip) — what can be checked without a GPU: the four
entry points are declared, exported and mirrored in the Rust FFI; ragged.hip compiles for gfx950 within its resource targets;
the Python mirror validates before it touches a device; the tag table is compute_tag per length; the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers.percall import build_cpp_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
RAGGED = ("p252_hash_ragged", "p252_hash_ragged_truncated", "p252_hash_ragged_device", "p252_hash_ragged_truncated_device")


def test_ragged_symbols_declared_exported_and_in_sys_rs():
    from poseidon252_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read(), flags=re.S)
    assert re.search(r"#define P252_ABI_VERSION 9\b", open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read())
    L = ctypes.CDLL(_lib.LIB_PATH)
    sysrs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (p252_\w+)\((.*?)\)", sysrs)}
    for name in RAGGED:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
        arity = 10 if name.endswith("_device") else 8
        assert rust[name].count(":") == arity, (name, rust[name])
    assert _lib.lib().p252_abi_version() == 9
    lib_rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read())
    assert "pub fn digest_ragged(&self, messages: &[&[BlsScalar]])" in lib_rs and "p252_hash_ragged(" in lib_rs


@pytest.fixture(scope="module")
def ragged_resources():
    from poseidon252_amd import build as b
    b._gen_assets()
    out = os.path.join(CSRC, "_gen", "ragged_test.s")
    cmd = [b._hipcc()] + [f for f in b.HIPCC_FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                                      "-o", out, os.path.join(CSRC, "ragged.hip")]
    proc = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    r = proc.stderr
    names = re.findall(r"Function Name: (\S+)", r)
    cols = [[int(x) for x in re.findall(pat, r)] for pat in (r"\bVGPRs: (\d+)", r"\bAGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)",
                                                               r"Occupancy \[waves/SIMD\]: (\d+)")]
    assert all(len(c) == len(names) for c in cols), r[-2000:]
    return {n: dict(zip(("vgpr", "agpr", "scratch", "occ"), vals)) for n, *vals in zip(names, *cols)}


def test_ragged_kernels_meet_resource_targets(ragged_resources):
    res = ragged_resources
    short = {re.sub(r"^_ZN4p252\d+", "", n).split("E")[0]: v for n, v in res.items()}
    assert {"k_ragged_hist", "k_ragged_scan", "k_ragged_scatter", "k_sponge_ragged", "k_sponge_ragged_trunc", "k_sponge_ragged_coop",
            "k_sponge_ragged_coop_trunc"} <= set(short), sorted(short)
    for name, v in short.items():
        assert v["scratch"] == 0 and v["agpr"] == 0, (name, v)
    for name in ("k_sponge_ragged", "k_sponge_ragged_trunc"):  # the class of k_sponge: all five rows in VGPRs, two waves per SIMD
        assert short[name]["vgpr"] <= 256 and short[name]["occ"] >= 2, (name, short[name])
    for name in ("k_ragged_hist", "k_ragged_scan", "k_ragged_scatter"):
        assert short[name]["vgpr"] <= 64, (name, short[name])


def test_ragged_is_its_own_translation_unit():
    from poseidon252_amd import build as b
    assert "ragged.hip" in b.SOURCES and "ragged.h" in b.HEADERS
    assert "ragged" not in open(os.path.join(CSRC, "kernels.hip")).read()


def test_merkle_domains_are_refused():
    import poseidon252_amd as P
    for dom in (P.Domain.Merkle4, P.Domain.Merkle2):
        with pytest.raises(P.IOPatternViolation, match="HashBatch"):
            P.RaggedHashBatch(dom)
    assert P.RaggedHashBatch(P.Domain.Encryption, output_len=5).out_len == 1  # hash.rs:111-115: honoured for Domain::Other only
    assert P.RaggedHashBatch(P.Domain.Other, output_len=5).out_len == 5


def test_host_validation_before_any_device():
    """(no context is created: these raise on a machine without a GPU as well)"""
    import poseidon252_amd as P
    rb = P.RaggedHashBatch(P.Domain.Other, ctx=object())  # a context that would fail on any use
    with pytest.raises(P.InvalidIOPattern):
        rb.digest([np.zeros((3, 4), np.uint64), np.zeros((0, 4), np.uint64)])
    with pytest.raises(P.InvalidIOPattern):
        rb.digest((np.zeros((6, 4), np.uint64), np.array([0, 3, 3, 6], np.uint64)))
    with pytest.raises(ValueError, match="decrease"):
        rb.digest((np.zeros((6, 4), np.uint64), np.array([0, 4, 2, 6], np.uint64)))
    with pytest.raises(ValueError, match="max_len"):
        rb.digest([np.zeros((5, 4), np.uint64)], max_len=4)
    with pytest.raises(ValueError, match="past"):
        rb.digest((np.zeros((6, 4), np.uint64), np.array([0, 3, 7], np.uint64)))
    assert rb.digest([]).shape == (0, 1, 4)


def test_tag_table_is_compute_tag_per_length_and_cached():
    import poseidon252_amd as P
    from poseidon252_amd import hash as H
    for dom, out_len in ((P.Domain.Other, 1), (P.Domain.Other, 5), (P.Domain.Encryption, 1)):
        rb = P.RaggedHashBatch(dom, output_len=out_len)
        t = rb.tags(45)
        assert t.shape == (45, 4) and t.dtype == np.uint64
        for L in range(1, 46):
            assert np.array_equal(t[L - 1], P.compute_tag(dom, [L], out_len)), (dom, out_len, L)
        assert rb.tags(45) is t and H.ragged_tags(dom, out_len, 45) is t
    # a chunked update aggregates to the one-shot tag (test_hash_api), so one table per total length serves any chunking
    assert np.array_equal(P.compute_tag(P.Domain.Other, [3, 39], 5), P.RaggedHashBatch(P.Domain.Other, output_len=5).tags(42)[41])


def test_ragged_call_without_gpu_raises_device_error():
    import torch
    import poseidon252_amd as P
    if torch.cuda.is_available():
        pytest.skip("GPU present (tests/test_ragged_gpu.py)")
    with pytest.raises(P.DeviceError):
        P.RaggedHashBatch(P.Domain.Other).digest([np.zeros((3, 4), np.uint64), np.zeros((5, 4), np.uint64)])


def test_cpp_mirror_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_ragged_api", tmp_path)


def test_ragged_bench_tool_parses():
    src = open(os.path.join(ROOT, "bench_tools", "ragged_bench.py")).read()
    compile(src, "ragged_bench.py", "exec")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "ragged_bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--messages" in r.stdout, r.stderr
