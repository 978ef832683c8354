"""Openings out of a forest of trees of different sizes (p252_merkle{4,2}_forest_ragged_openings_device, p252_merkle{4,2}_path_ragged_device,
p252_merkle{4,2}_forest_ragged_verify_device; csrc/forest_openings.hip) — what can be checked without a GPU: the six entry points are
declared, exported and mirrored in the Rust FFI under ABI 9; forest_openings.hip compiles for gfx950 within its resource targets and
includes the library's permutation instead of copying it; the Python mirror validates every buffer before it reaches the library; a
stale ABI-9 build is reported by name; the C++ mirror test compiles."""
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers.binding import _dev, recorder  # noqa: F401
from helpers.kernel_resources import kernel_resources
from helpers.percall import bench_tool_parses, build_cpp_mirror, check_abi_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
ARGS = {"p252_merkle4_forest_ragged_openings_device": 16, "p252_merkle2_forest_ragged_openings_device": 16,
        "p252_merkle4_path_ragged_device": 11, "p252_merkle2_path_ragged_device": 11,
        "p252_merkle4_forest_ragged_verify_device": 13, "p252_merkle2_forest_ragged_verify_device": 13}


def test_six_symbols_declared_exported_and_in_sys_rs():
    check_abi_symbols(ARGS)


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("forest_openings.hip", os.path.join(CSRC, "_gen", "forest_openings_test.s"))[0]


def test_kernels_meet_resource_targets(resources):
    res = resources
    path = {n: v for n, v in res.items() if "k_path_ragged" in n}
    pieces = {n: v for n, v in res.items() if "k_fr_openings" in n}
    assert len(path) == 2 and len(pieces) == 4, sorted(res)  # both arities; both arities x both index widths
    for want in ("k_fo_record", "k_fo_depth_hist", "k_fo_depth_scan", "k_fo_depth_scatter", "k_compare_roots_gather"):
        assert any(want in n for n in res), (want, sorted(res))
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0, (name, v)
    for name, v in path.items():  # k_merkle4's target: three waves per SIMD
        assert v["occ"] == 3, (name, v)
    for name, v in res.items():
        if "k_path_ragged" not in name:  # the extraction, sort, compare and record kernels are small
            assert v["vgpr"] <= 64, (name, v)


def test_own_translation_unit_and_the_permutation_is_included():
    from poseidon252_amd import build as b
    assert "forest_openings.hip" in b.SOURCES and "forest_openings.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_openings.hip")).read()
    assert '#include "hades29.hpp"' in src and "hades_permute<0x02u, true>" in src
    assert "amdgpu_waves_per_eu(3, 3)" in src
    assert "forest_openings" not in open(os.path.join(CSRC, "kernels.hip")).read()
    assert "forest_openings" not in open(os.path.join(CSRC, "kernels.h")).read()
    # the forest's index comes from the build's own kernels, not from a copy of them
    assert "k_fr_prep" not in src and "launch_forest_ragged_index" in open(os.path.join(CSRC, "forest_ragged.hip")).read()


@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_validate_before_any_device_call(recorder, arity):
    from poseidon252_amd import Context
    ctx = Context.__new__(Context)  # no device: nothing below may reach one
    ctx._h, ctx.device = None, 0
    tag = np.zeros(4, dtype=np.uint64)
    per = arity - 1
    n_leaves, n_trees, max_leaves, k = 40, 3, 16, 5
    D = 2 if arity == 4 else 4
    u8, i32 = torch.uint8, torch.int32
    good = dict(d_leaves=_dev(n_leaves * 4), d_offsets=_dev(n_trees + 1), d_levels=_dev((n_leaves // per + n_trees * D) * 4),
                d_tree_ids=_dev(k, i32), d_leaf_ids=_dev(k), d_leaves_out=_dev(k * 4), d_siblings=_dev(k * D * per * 4),
                d_positions=_dev(k * D, u8), d_depths=_dev(k, u8), d_n_bad=_dev(1, i32), d_roots=_dev(k * 4), d_forest_roots=_dev(n_trees * 4),
                d_ok=_dev(k, u8))

    def openings(a):
        return ctx.merkle_forest_ragged_openings_device(a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_tree_ids"],
                                                        a["d_leaf_ids"], k, out=(a["d_leaves_out"], a["d_siblings"], a["d_positions"], a["d_depths"]),
                                                        d_n_bad=a["d_n_bad"], arity=arity)

    def path(a):
        return ctx.merkle_path_ragged_device(tag, a["d_leaves_out"], a["d_siblings"], a["d_positions"], a["d_depths"], D, a["d_roots"], k,
                                             d_n_bad=a["d_n_bad"], arity=arity)

    def verify(a):
        return ctx.merkle_forest_ragged_verify_device(tag, a["d_leaves_out"], a["d_siblings"], a["d_positions"], a["d_depths"], D,
                                                      a["d_tree_ids"], a["d_forest_roots"], n_trees, a["d_ok"], k, arity=arity)

    calls = {
        "p252_merkle%d_forest_ragged_openings_device" % arity: (openings, ["d_leaves", "d_offsets", "d_levels", "d_tree_ids", "d_leaf_ids", "d_leaves_out",
                                                                            "d_siblings", "d_positions", "d_depths", "d_n_bad"]),
        "p252_merkle%d_path_ragged_device" % arity: (path, ["d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_roots", "d_n_bad"]),
        "p252_merkle%d_forest_ragged_verify_device" % arity: (verify, ["d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_tree_ids",
                                                                       "d_forest_roots", "d_ok"]),
    }
    wrong_dtype = {"d_offsets": i32, "d_tree_ids": torch.int64, "d_leaf_ids": i32, "d_positions": i32, "d_depths": i32, "d_n_bad": torch.int64,
                   "d_ok": i32}
    n_refused = 0
    for symbol, (call, names) in calls.items():
        call(good)
        assert recorder.calls == [symbol], (symbol, recorder.calls)  # the control: all good -> the library is reached, once
        del recorder.calls[:]
        for name in names:
            t = good[name]
            variants = [("is on cpu", torch.zeros_like(t.as_subclass(torch.Tensor))),                     # a host tensor
                        ("holds", t[:max(t.numel() - 1, 0)] if t.numel() > 1 else _dev(0, t.dtype)),       # one element short
                        ("not contiguous", _dev(2 * t.numel(), t.dtype)[::2]),                              # a strided view
                        ("torch tensor", np.zeros(t.numel()))]                                              # no tensor at all
            if name == "d_leaves":  # (its length IS the forest's leaf count: any tensor of one scalar or more is taken)
                variants = [v for v in variants if v[0] != "holds"]
            if t.numel() == 1:  # (a one-element view is contiguous whatever its stride)
                variants = [v for v in variants if v[0] != "not contiguous"]
            if name in wrong_dtype:
                variants.append(("-byte elements", _dev(t.numel() * 8, wrong_dtype[name])))
            for match, bad in variants:
                with pytest.raises(ValueError, match=match):
                    call(dict(good, **{name: bad}))
                assert recorder.calls == [], (symbol, name, match)
                n_refused += 1
    assert n_refused >= 90
    g = good
    for bad_arity in (lambda: ctx.merkle_forest_ragged_openings_device(g["d_leaves"], g["d_offsets"], n_trees, max_leaves, g["d_levels"],
                                                                       g["d_tree_ids"], g["d_leaf_ids"], k, arity=3),
                      lambda: ctx.merkle_path_ragged_device(tag, g["d_leaves_out"], g["d_siblings"], g["d_positions"], g["d_depths"], D,
                                                            g["d_roots"], k, arity=3),
                      lambda: ctx.merkle_forest_ragged_verify_device(tag, g["d_leaves_out"], g["d_siblings"], g["d_positions"], g["d_depths"], D,
                                                                     g["d_tree_ids"], g["d_forest_roots"], n_trees, g["d_ok"], k, arity=3)):
        with pytest.raises(ValueError, match="arity"):
            bad_arity()
    with pytest.raises(ValueError, match="stride_depth"):
        ctx.merkle_path_ragged_device(tag, good["d_leaves_out"], good["d_siblings"], good["d_positions"], good["d_depths"], 65, good["d_roots"], k,
                                      arity=arity)
    assert recorder.calls == []


def test_stale_abi9_build_is_reported_by_name(tmp_path, monkeypatch):
    """a library that reports ABI 9 but was built before these entry points: ExtensionMissing naming the symbol, not AttributeError"""
    from poseidon252_amd import _lib
    stubs = ["int %s(void) { return %d; }" % (n, 9 if n == "p252_abi_version" else 0) for n in _lib.ABI_SYMBOLS if n not in ARGS]
    src = tmp_path / "stale.c"
    src.write_text("\n".join(stubs) + "\n")
    so = str(tmp_path / "libstale.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", so, str(src)])
    monkeypatch.delenv("P252_LIB_PATH", raising=False)
    monkeypatch.setattr(_lib, "LIB_PATH", so)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.ExtensionMissing, match="rebuild") as e:
        _lib.lib()
    assert "p252_merkle4_forest_ragged_openings_device" in str(e.value)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_openings_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_openings_bench", options=("--openings",))
