"""Many leaves of ONE stored tree behind one shared proof (p252_merkle{4,2}_multiproof_bound / _device / _verify_device;
csrc/multiproof.hip) — what can be checked without a GPU: the six entry points are declared, exported and mirrored in the Rust FFI
under ABI 9; multiproof.hip compiles for gfx950 within its resource targets and includes the library's permutation instead of
copying it; the numpy model of the format that the GPU tests compare the device's bytes with agrees with a brute-force set
construction and, with the oracle's digest, reproduces the oracle's roots; the bound holds and is tight for one leaf; the Python
mirror validates every buffer before it reaches the library; the C++ mirror test compiles."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from helpers.binding import _dev, recorder  # noqa: E402,F401  (the stub library and the tensors that pass for device ones)
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import bench_tool_parses, build_cpp_mirror, check_abi_symbols  # noqa: E402
from testsupport.multiproofmodel import multiproof_bound, multiproof_counts, multiproof_extract, multiproof_model, multiproof_root  # noqa: E402

ARGS = {"p252_merkle4_multiproof_bound": 2, "p252_merkle2_multiproof_bound": 2,
        "p252_merkle4_multiproof_device": 12, "p252_merkle2_multiproof_device": 12,
        "p252_merkle4_multiproof_verify_device": 14, "p252_merkle2_multiproof_verify_device": 14}
SHAPES = [(4, n) for n in (1, 2, 4, 5, 16, 17, 21, 64, 1000)] + [(2, n) for n in (1, 2, 3, 7, 33, 1000)]  # the GPU test's


def test_six_symbols_declared_exported_and_in_sys_rs():
    check_abi_symbols(ARGS)


@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("multiproof.hip", os.path.join(CSRC, "_gen", "multiproof_test.s"))


def test_kernels_meet_resource_targets(compiled):
    res, isa = compiled
    one_lane = {n: v for n, v in res.items() if "k_mp_digestI" in n}
    coop = {n: v for n, v in res.items() if "k_mp_digest_coop" in n}
    book = {n: v for n, v in res.items() if "k_mp_digest" not in n}
    assert len(one_lane) == 2 and len(coop) == 2, sorted(res)  # both arities
    for want, count in (("k_mp_check", 1), ("k_mp_tile_sums", 2), ("k_mp_scan_tiles", 1), ("k_mp_apply", 4), ("k_mp_finish", 2)):
        assert sum(want in n for n in book) == count, (want, sorted(book))  # both arities; the apply with and without the copies
    assert len(res) == 14, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0, (name, v)
    for name, v in one_lane.items():  # k_merkle4's target: three waves per SIMD
        assert v["occ"] >= 3, (name, v)
    for name, v in book.items():
        assert v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_own_translation_unit_and_the_permutation_is_included():
    from poseidon252_amd import build as b
    assert "multiproof.hip" in b.SOURCES and "multiproof.h" in b.HEADERS
    src = open(os.path.join(CSRC, "multiproof.hip")).read()
    assert '#include "forest_node.hpp"' in src and '#include "hades29.hpp"' in src
    assert "hades_permute<0x02u, true>" in src and "node_digest_coop<ARITY>(" in src and "coop8(" in src
    assert not re.search(r"\bhades_\w+\s*\([^;{]*\)\s*\{", src)  # no hades_* function is defined here
    assert "hades_permute_coop" not in src  # the 8-lane schedule is forest_node.hpp's
    assert "amdgpu_waves_per_eu(3, 3)" in src
    assert "asm" not in src  # plain C++ and vector stores only
    for other in ("kernels.hip", "kernels.h", "forest_update.hip", "forest_ragged.hip", "forest_node.hpp"):
        assert "multiproof" not in open(os.path.join(CSRC, other)).read(), other
    assert not re.search(r"\bk_f[ru]_\w+\s*[(<]", src)  # its scan is its own


def _brute(n, positions, arity):
    """the format, read off the issue's wording with sets: (proof nodes per level in visiting order, digests)"""
    S, w, proof, hashed = set(int(p) for p in positions), n, [], 0
    while w > 1:
        parents = sorted({i // arity for i in S})
        level = []
        for p in parents:
            for c in range(p * arity, p * arity + arity):
                if c < w and c not in S:
                    level.append(c)
        proof.append(level)
        hashed += len(parents)
        S, w = set(parents), (w + arity - 1) // arity
    return proof, hashed


def _index_sets(n, rng):
    sets = [[0], [n - 1], sorted({0, n - 1}), list(range(0, n, 2)), list(range(n)), [0, 1] if n > 1 else [0]]
    for k in {1, max(1, n // 7), max(1, n // 2), max(1, n - 1)}:
        sets.append(np.sort(rng.choice(n, k, replace=False)).tolist())
    return sets


def test_model_agrees_with_a_brute_force_set_construction_and_the_bound_holds():
    from poseidon252_amd import _lib, levels_len
    L = _lib.lib()
    rng = np.random.default_rng(3)
    for arity in (4, 2):
        bound_fn = L.p252_merkle4_multiproof_bound if arity == 4 else L.p252_merkle2_multiproof_bound
        for n in (1, 2, 3, 4, 5, 7, 16, 17, 21, 33, 64, 65, 1000, 4099):
            for pos in _index_sets(n, rng):
                nodes, S, w = multiproof_model(n, pos, arity)
                want, hashed = _brute(n, pos, arity)
                assert [x.tolist() for x in nodes] == want, (arity, n, pos)
                assert multiproof_counts(n, pos, arity) == (sum(len(x) for x in want), hashed)
                assert w[-1] == 1 and S[-1].tolist() == [0] and len(w) == len(S)
                bound = bound_fn(n, len(pos))
                assert bound == multiproof_bound(n, len(pos), arity) >= sum(len(x) for x in want), (arity, n, len(pos))
            assert multiproof_counts(n, list(range(n)), arity) == (0, levels_len(n, arity))  # every leaf: no proof, every node hashed
        for d in range(0, 7):  # one leaf of a complete tree: the bound is reached
            n = arity ** d
            assert multiproof_counts(n, [n // 3], arity)[0] == bound_fn(n, 1) == d * (arity - 1)
        assert bound_fn(0, 5) == 0 and bound_fn(5, 0) == 0


@pytest.mark.parametrize("arity,n", SHAPES)
def test_model_with_the_oracles_digest_gives_the_oracles_root(oracle_mod, arity, n):
    from poseidon252_amd import merkle as M
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    leaves = oracle_mod.fill_random(40 + n, n)
    root, levels = (oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree)(tag, leaves, want_levels=True)[:2]
    digest = lambda x: oracle_mod.hash_batch(tag, x, arity, 1)  # noqa: E731
    rng = np.random.default_rng(n)
    for pos in _index_sets(n, rng)[:8]:
        proof = multiproof_extract(leaves, levels, pos, arity)
        assert np.array_equal(multiproof_root(n, pos, leaves[pos], proof, arity, digest), root), (arity, n, pos)
        if proof.shape[0]:
            changed = proof.copy()
            changed[proof.shape[0] // 2, 2] ^= np.uint64(1)
            assert not np.array_equal(multiproof_root(n, pos, leaves[pos], changed, arity, digest), root)
            assert multiproof_root(n, pos, leaves[pos], proof[:-1], arity, digest) is None
        assert multiproof_root(n, pos, leaves[pos], np.concatenate([proof, leaves[:1]]), arity, digest) is None


@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_validate_before_any_device_call(recorder, arity):
    from poseidon252_amd import Context, levels_len
    ctx = Context.__new__(Context)  # no device: nothing below may reach one
    ctx._h, ctx.device = None, 0
    tag = np.zeros(4, dtype=np.uint64)
    n, k, cap = 40, 5, 12
    i32, u8 = torch.int32, torch.uint8
    good = dict(d_leaves=_dev(n * 4), d_levels=_dev(levels_len(n, arity) * 4), d_indices=_dev(k, i32), d_leaves_out=_dev(k * 4),
                d_proof=_dev(cap * 4), d_proof_len=_dev(1), d_n_bad=_dev(1, i32), d_leaves_in=_dev(k * 4), d_root=_dev(4), d_ok=_dev(1, u8),
                d_root_out=_dev(4), d_n_hashed=_dev(1))

    def extract(a, k=k, arity=arity):
        return ctx.merkle_multiproof_device(a["d_leaves"], n, a["d_levels"], a["d_indices"], k, a["d_leaves_out"], a["d_proof"],
                                            a["d_proof_len"], d_n_bad=a["d_n_bad"], arity=arity)

    def verify(a, k=k, arity=arity, proof_len=cap):
        return ctx.merkle_multiproof_verify_device(tag, n, a["d_indices"], a["d_leaves_in"], k, a["d_proof"], proof_len, a["d_root"], a["d_ok"],
                                                   d_root_out=a["d_root_out"], d_n_hashed=a["d_n_hashed"], d_n_bad=a["d_n_bad"], arity=arity)
    calls = {extract: ("p252_merkle%d_multiproof_device" % arity, ["d_leaves", "d_levels", "d_indices", "d_leaves_out", "d_proof", "d_proof_len", "d_n_bad"]),
             verify: ("p252_merkle%d_multiproof_verify_device" % arity, ["d_indices", "d_leaves_in", "d_proof", "d_root", "d_ok", "d_root_out",
                                                                         "d_n_hashed", "d_n_bad"])}
    wrong_dtype = {"d_indices": torch.int64, "d_proof_len": i32, "d_n_bad": torch.int64, "d_n_hashed": i32, "d_ok": i32}
    n_refused = 0
    for call, (symbol, names) in calls.items():
        call(good)
        assert recorder.calls == [symbol]  # the control: all good -> the library is reached, once
        del recorder.calls[:]
        call(dict(good, d_n_bad=None, d_root_out=None, d_n_hashed=None))  # the optional ones
        assert recorder.calls == [symbol]
        del recorder.calls[:]
        for name in names:
            t = good[name]
            variants = [("is on cpu", torch.zeros_like(t.as_subclass(torch.Tensor))),                     # a host tensor
                        ("holds", t[:max(t.numel() - 1, 0)] if t.numel() > 1 else _dev(0, t.dtype)),       # one element short
                        ("not contiguous", _dev(2 * t.numel(), t.dtype)[::2]),                              # a strided view
                        ("torch tensor", np.zeros(t.numel()))]                                              # no tensor at all
            if name == "d_proof" and call is extract:  # (its length IS the capacity: any tensor is taken)
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
        with pytest.raises(ValueError, match="holds"):  # k larger than the arrays
            call(good, k=k + 1)
        with pytest.raises(ValueError, match="arity"):
            call(good, arity=3)
        assert recorder.calls == []
    assert n_refused >= 45
    with pytest.raises(ValueError, match="holds"):  # a proof_len past the tensor
        verify(good, proof_len=cap + 1)
    with pytest.raises(ValueError, match="torch tensor"):  # a proof_len without a proof
        verify(dict(good, d_proof=None), proof_len=1)
    assert recorder.calls == []
    verify(dict(good, d_proof=None), proof_len=0)  # an empty proof needs no tensor
    extract(dict(good, d_proof=None))              # and a capacity of zero reports the length
    assert len(recorder.calls) == 2
    with pytest.raises(ValueError, match="arity"):
        ctx.merkle_multiproof_bound(5, 1, arity=3)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_multiproof_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("multiproof_bench")
