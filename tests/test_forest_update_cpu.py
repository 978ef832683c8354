"""Leaf updates anywhere in a forest of trees of different sizes (p252_merkle{4,2}_forest_ragged_update_device; csrc/forest_update.hip)
— what can be checked without a GPU: the two entry points are declared, exported and mirrored in the Rust FFI under ABI 9;
forest_update.hip compiles for gfx950 within its resource targets and includes the library's permutation instead of copying it;
the Python mirror validates every buffer before it reaches the library; the numpy model of the dirty-node count that the GPU tests
compare d_n_hashed with agrees with a brute-force set; the C++ mirror test compiles."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from helpers.binding import _dev, recorder  # noqa: F401  (the stub library and the tensors that pass for device ones)
from helpers.forest import dirty_count  # (the numpy model of what one call may hash; checked below)
from helpers.kernel_resources import kernel_resources
from helpers.percall import bench_tool_parses, build_cpp_mirror, check_abi_symbols

ARGS = {"p252_merkle4_forest_ragged_update_device": 16, "p252_merkle2_forest_ragged_update_device": 16}


def test_two_symbols_declared_exported_and_in_sys_rs():
    raw, _ = check_abi_symbols(ARGS)
    assert "no host-buffer twin" in raw  # the call acts on a forest that lives on the device, and the header says so


@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_update.hip", os.path.join(CSRC, "_gen", "forest_update_test.s"))


def test_kernels_meet_resource_targets(compiled):
    res, isa = compiled
    one_lane = {n: v for n, v in res.items() if "k_fu_digestI" in n}
    coop = {n: v for n, v in res.items() if "k_fu_digest_coop" in n}
    book = {n: v for n, v in res.items() if "k_fu_scatter" in n or "k_fu_claim" in n}
    assert len(one_lane) == 2 and len(coop) == 2 and len(book) == 2, sorted(res)  # both arities; the scatter and the claim
    assert len(res) == 6, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0, (name, v)
    for name, v in one_lane.items():  # k_merkle4's target: three waves per SIMD
        assert v["occ"] >= 3, (name, v)
    for name, v in book.items():
        assert v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_own_translation_unit_and_the_permutation_is_included():
    from poseidon252_amd import build as b
    assert "forest_update.hip" in b.SOURCES and "forest_update.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_update.hip")).read()
    node = open(os.path.join(CSRC, "forest_node.hpp")).read()
    # through forest_node.hpp, which holds the 8-lane digest of a node (the one-lane digest is written out in the kernel)
    assert "forest_node.hpp" in b.HEADERS and '#include "forest_node.hpp"' in src
    assert '#include "hades29.hpp"' in src and '#include "hades29.hpp"' in node and '#include "coop29.hpp"' in node
    assert "hades_permute<0x02u, true>" in src and "hades_permute_coop<8, false>" in node and "node_digest_coop<ARITY>(" in src
    assert not re.search(r"\bhades_\w+\s*\([^;{]*\)\s*\{", src)
    assert "amdgpu_waves_per_eu(3, 3)" in src
    assert "asm" not in src  # plain C++ and vector stores only
    assert "forest_update" not in open(os.path.join(CSRC, "kernels.hip")).read()
    assert "forest_update" not in open(os.path.join(CSRC, "kernels.h")).read()
    # the forest's index comes from the build's own kernels, not from a copy of them
    assert not re.search(r"\bk_fr_\w+\s*[(<]", src) and "launch_forest_ragged_index" in open(os.path.join(CSRC, "api_forest.cpp")).read()


@pytest.mark.parametrize("arity", [4, 2])
def test_python_method_validates_before_any_device_call(recorder, arity):
    from poseidon252_amd import Context
    ctx = Context.__new__(Context)  # no device: nothing below may reach one
    ctx._h, ctx.device = None, 0
    tag = np.zeros(4, dtype=np.uint64)
    n_leaves, n_trees, max_leaves, k = 40, 3, 16, 5
    D = 2 if arity == 4 else 4
    i32 = torch.int32
    good = dict(d_leaves=_dev(n_leaves * 4), d_offsets=_dev(n_trees + 1), d_levels=_dev((n_leaves // (arity - 1) + n_trees * D) * 4),
                d_tree_ids=_dev(k, i32), d_leaf_ids=_dev(k), d_new_leaves=_dev(k * 4), d_roots=_dev(n_trees * 4), d_n_bad=_dev(1, i32),
                d_n_hashed=_dev(1))

    def call(a, k=k, arity=arity):
        return ctx.merkle_forest_ragged_update_device(tag, a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_tree_ids"],
                                                      a["d_leaf_ids"], a["d_new_leaves"], k, d_roots=a["d_roots"], d_n_bad=a["d_n_bad"],
                                                      d_n_hashed=a["d_n_hashed"], arity=arity)
    symbol = "p252_merkle%d_forest_ragged_update_device" % arity
    call(good)
    assert recorder.calls == [symbol]  # the control: all good -> the library is reached, once
    del recorder.calls[:]
    call(dict(good, d_roots=None, d_n_bad=None, d_n_hashed=None))  # the three optional ones
    assert recorder.calls == [symbol]
    del recorder.calls[:]
    wrong_dtype = {"d_offsets": i32, "d_tree_ids": torch.int64, "d_leaf_ids": i32, "d_n_bad": torch.int64, "d_n_hashed": i32}
    n_refused = 0
    for name, t in good.items():
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
            assert recorder.calls == [], (name, match)
            n_refused += 1
    assert n_refused >= 35
    with pytest.raises(ValueError, match="holds"):  # k larger than the id arrays
        call(good, k=k + 1)
    with pytest.raises(ValueError, match="arity"):
        call(good, arity=3)
    assert recorder.calls == []


def test_dirty_count_model_agrees_with_a_brute_force_set():
    rng = np.random.default_rng(9)
    for arity in (4, 2):
        sizes = [1, 2, 3, arity, arity + 1, arity * arity + 1, 0, 63, 65, 300]
        for k in (1, 7, 60, 400):
            tid = rng.integers(0, len(sizes) + 2, k)  # (ids past the forest among them)
            lid = rng.integers(0, 70, k)              # (ids past the small trees among them, and repeats)
            seen = set()
            for t, leaf in zip(tid.tolist(), lid.tolist()):
                if t >= len(sizes) or leaf >= sizes[t]:
                    continue
                n, i, level = sizes[t], leaf, 0
                while n > 1:
                    n, i, level = (n + arity - 1) // arity, i // arity, level + 1
                    seen.add((t, level, i))
            assert dirty_count(sizes, tid, lid, arity) == len(seen), (arity, k)
    # every leaf of every tree: every node of the forest
    from poseidon252_amd import levels_len
    sizes = [1, 5, 17, 256, 1000]
    tid = np.repeat(np.arange(len(sizes)), sizes)
    lid = np.concatenate([np.arange(n) for n in sizes])
    for arity in (4, 2):
        assert dirty_count(sizes, tid, lid, arity) == sum(levels_len(n, arity) for n in sizes)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_update_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_update_bench")
