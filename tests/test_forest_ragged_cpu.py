"""A forest of Merkle trees of different sizes in one call (p252_merkle{4,2}_forest_ragged*, csrc/forest_ragged.hip) — what can be
checked without a GPU: the four entry points are declared, exported and mirrored in the Rust FFI under ABI 9; forest_ragged.hip
compiles for gfx950 within its resource targets; the Python mirror validates before it touches a device and lays out the levels
by the single-tree sizes; a stale ABI-9 build is reported by name; the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers.kernel_resources import kernel_resources
from helpers.percall import bench_tool_parses, build_cpp_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
FOREST = ("p252_merkle4_forest_ragged_device", "p252_merkle2_forest_ragged_device", "p252_merkle4_forest_ragged",
          "p252_merkle2_forest_ragged")


def test_forest_ragged_symbols_declared_exported_and_in_sys_rs():
    from poseidon252_amd import _lib
    raw = open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define P252_ABI_VERSION 9\b", raw)
    L = ctypes.CDLL(_lib.LIB_PATH)
    sysrs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (p252_\w+)\((.*?)\)", sysrs)}
    for name in FOREST:
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        n_args = m.group(1).count(",") + 1
        assert n_args == (11 if name.endswith("_device") else 7), (name, n_args)
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
        assert len(_lib.PROTOTYPES[name][0]) == n_args, name
        assert rust[name].count(":") == n_args, (name, rust[name])
    assert _lib.lib().p252_abi_version() == 9 and _lib.ABI_VERSION == 9


@pytest.fixture(scope="module")
def forest_resources():
    return kernel_resources("forest_ragged.hip", os.path.join(CSRC, "_gen", "forest_ragged_test.s"))[0]


def test_forest_ragged_kernels_meet_resource_targets(forest_resources):
    res = forest_resources
    digest = {n: v for n, v in res.items() if "k_fr_digest" in n and "coop" not in n}
    coop = {n: v for n, v in res.items() if "k_fr_digest_coop" in n}
    assert len(digest) == 2 and len(coop) == 2, sorted(res)  # both arities of both builds
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0, (name, v)
    for name, v in digest.items():  # k_merkle4's target: three waves per SIMD
        assert v["occ"] == 3, (name, v)
    for name, v in res.items():
        if "k_fr_digest" not in name:  # the prep / scan / lookup kernels are small
            assert v["vgpr"] <= 64, (name, v)


def test_forest_ragged_is_its_own_translation_unit_and_the_hashed_sources_stay():
    from poseidon252_amd import build as b
    assert "forest_ragged.hip" in b.SOURCES and "forest_ragged.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_ragged.hip")).read()
    node = open(os.path.join(CSRC, "forest_node.hpp")).read()
    # the permutation is included, not copied: through forest_node.hpp, which holds the 8-lane digest of a node (the one-lane
    # digest is written out in the kernel); no function named hades_* is defined here
    assert "forest_node.hpp" in b.HEADERS and '#include "forest_node.hpp"' in src
    assert '#include "hades29.hpp"' in src and '#include "hades29.hpp"' in node and '#include "coop29.hpp"' in node
    assert "hades_permute<0x02u, true>" in src and "hades_permute_coop<8, false>" in node and "node_digest_coop<ARITY>(" in src
    assert not re.search(r"\bhades_\w+\s*\([^;{]*\)\s*\{", src)
    assert "forest_ragged" not in open(os.path.join(CSRC, "kernels.hip")).read()
    assert "forest_ragged" not in open(os.path.join(CSRC, "kernels.h")).read()


def test_python_mirror_validates_before_any_device():
    """(the context given would fail on any use: these raise on a machine without a GPU as well)"""
    import poseidon252_amd as P
    no_ctx = object()
    with pytest.raises(ValueError, match="empty"):
        P.merkle_forest_ragged([np.zeros((3, 4), np.uint64), np.zeros((0, 4), np.uint64)], ctx=no_ctx)
    with pytest.raises(ValueError, match="empty"):
        P.merkle_forest_ragged((np.zeros((6, 4), np.uint64), np.array([0, 3, 3, 6], np.uint64)), ctx=no_ctx)
    with pytest.raises(ValueError, match="decrease"):
        P.merkle_forest_ragged((np.zeros((6, 4), np.uint64), np.array([0, 4, 2, 6], np.uint64)), ctx=no_ctx)
    with pytest.raises(ValueError, match="past"):
        P.merkle_forest_ragged((np.zeros((6, 4), np.uint64), np.array([0, 3, 7], np.uint64)), ctx=no_ctx)
    with pytest.raises(ValueError, match="uint64"):
        P.merkle_forest_ragged([np.zeros((3, 4), np.float64)], ctx=no_ctx)
    with pytest.raises(ValueError, match="uint64"):
        P.merkle_forest_ragged((np.zeros((6, 4), np.uint64), np.array([0, 3, 6], np.float32)), ctx=no_ctx)
    with pytest.raises(ValueError, match="arity"):
        P.merkle_forest_ragged([np.zeros((3, 4), np.uint64)], arity=3, ctx=no_ctx)
    assert P.merkle_forest_ragged([], ctx=no_ctx).shape == (0, 4)


class _RecordingCtx:
    """stands in for a Context: records the host call and returns zero roots / levels of the size asked for"""

    def __init__(self, lib, arity):
        self.ll = lib.p252_merkle4_levels_len if arity == 4 else lib.p252_merkle2_levels_len
        self.calls = []

    def merkle_forest_ragged(self, tag, flat, off, arity=4, want_levels=False):
        self.calls.append((tag, flat, off, arity, want_levels))
        n = off.shape[0] - 1
        total = sum(self.ll(int(off[t + 1] - off[t])) for t in range(n))
        return np.zeros((n, 4), np.uint64), np.zeros((total, 4), np.uint64)


@pytest.mark.parametrize("arity", [4, 2])
def test_level_offsets_are_the_prefix_sums_of_levels_len(arity):
    import poseidon252_amd as P
    from poseidon252_amd import _lib
    L = _lib.lib()
    ll = L.p252_merkle4_levels_len if arity == 4 else L.p252_merkle2_levels_len
    sizes = [1, 2, 3, arity, arity + 1, 63, 65, 1025, 16, 17]
    trees = [np.full((n, 4), k, np.uint64) for k, n in enumerate(sizes)]
    ctx = _RecordingCtx(L, arity)
    roots, levels, lo = P.merkle_forest_ragged(trees, arity=arity, ctx=ctx, want_levels=True)
    exp = np.concatenate([[0], np.cumsum([ll(n) for n in sizes])]).astype(np.uint64)
    assert lo.dtype == np.uint64 and np.array_equal(lo, exp)
    assert roots.shape == (len(sizes), 4) and levels.shape == (int(exp[-1]), 4)
    assert [P.levels_len(n, arity) for n in sizes] == [ll(n) for n in sizes]
    tag, flat, off, a, want = ctx.calls[0]
    assert a == arity and want and np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    assert np.array_equal(flat[:, 0], np.repeat(np.arange(len(sizes)), sizes).astype(np.uint64))
    from poseidon252_amd import merkle as M
    assert np.array_equal(tag, M.merkle4_tag() if arity == 4 else M.merkle2_tag())


def test_stale_abi9_build_is_reported_by_name(tmp_path, monkeypatch):
    """a library that reports ABI 9 but was built before these entry points: ExtensionMissing naming the symbol, not AttributeError"""
    from poseidon252_amd import _lib
    stubs = ["int %s(void) { return %d; }" % (n, 9 if n == "p252_abi_version" else 0) for n in _lib.ABI_SYMBOLS if n not in FOREST]
    src = tmp_path / "stale.c"
    src.write_text("\n".join(stubs) + "\n")
    so = str(tmp_path / "libstale.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", so, str(src)])
    monkeypatch.delenv("P252_LIB_PATH", raising=False)
    monkeypatch.setattr(_lib, "LIB_PATH", so)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.ExtensionMissing, match="rebuild") as e:
        _lib.lib()
    assert "p252_merkle4_forest_ragged_device" in str(e.value)


def test_cpp_mirror_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_ragged_api", tmp_path)


def test_forest_ragged_bench_tool_parses():
    bench_tool_parses("forest_ragged_bench", options=("--w2-trees",))
