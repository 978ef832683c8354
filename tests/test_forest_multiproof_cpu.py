"""The shared proof across a ragged forest (p252_merkle{4,2}_forest_ragged_multiproof_bound / _device / _verify_device;
csrc/forest_multiproof.hip) — what can be checked without a GPU: the six entry points are declared, exported and mirrored in the Rust
FFI under ABI 9; forest_multiproof.hip is its own translation unit, compiles for gfx950 within its resource targets and holds no
hashing kernel; the model the GPU tests compare the device's bytes with (a composition of the single-tree model) agrees with a
brute-force set construction and, with the oracle's digest, reproduces the oracle's roots; the bound holds and is reached; the Python
mirror validates every buffer before it reaches the library; every host refusal is the recorded one; the C++ mirror test compiles."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from helpers.binding import _dev, recorder  # noqa: E402,F401  (the stub library and the tensors that pass for device ones)
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import (ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols,  # noqa: E402
                             refusal_table)
from testsupport.multiproofmodel import (forest_multiproof_bound, forest_multiproof_counts, forest_multiproof_extract,  # noqa: E402
                             forest_multiproof_roots)
import edgecases as E  # noqa: E402

ARGS = {"p252_merkle4_forest_ragged_multiproof_bound": 4, "p252_merkle2_forest_ragged_multiproof_bound": 4,
        "p252_merkle4_forest_ragged_multiproof_device_into": 16, "p252_merkle2_forest_ragged_multiproof_device_into": 16,
        "p252_merkle4_forest_ragged_multiproof_verify_device_into": 19, "p252_merkle2_forest_ragged_multiproof_verify_device_into": 19}
SIZES = (0, 1, 2, 3, 4, 5, 16, 17, 21, 64, 65)


def test_six_symbols_declared_exported_and_in_sys_rs():
    check_abi_symbols(ARGS)


def test_own_translation_unit_without_a_hashing_kernel():
    from poseidon252_amd import build as b
    assert "forest_multiproof.hip" in b.SOURCES and "forest_multiproof.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_multiproof.hip")).read()
    assert "asm" not in src  # plain C++ and vector stores only
    assert "launch_multiproof_digest_list(" in src and "launch_forest_ragged_index(" in src
    mine = set(re.findall(r"\b(k_fm_\w+)\s*\(", re.sub(r"//[^\n]*", "", src)))
    assert len(mine) >= 8, sorted(mine)
    assert not (E.hashing_kernels() & mine)  # the digests are multiproof.hip's kernels
    assert not any(k.startswith("k_fm_") for k in E.hashing_kernels())
    for other in ("kernels.hip", "kernels.h", "forest_update.hip", "forest_ragged.hip", "forest_node.hpp"):
        assert "multiproof" not in open(os.path.join(CSRC, other)).read(), other


def test_kernels_meet_resource_targets():
    res, isa = kernel_resources("forest_multiproof.hip", os.path.join(CSRC, "_gen", "forest_multiproof_test.s"))
    for want, count in (("k_fm_check", 1), ("k_fm_tile_sums", 2), ("k_fm_scan_tiles", 1), ("k_fm_apply", 4), ("k_fm_tree_", 3),
                        ("k_fm_finish_verify", 1)):
        assert sum(want in n for n in res) == count, (want, sorted(res))  # both arities; the apply with and without the copies
    assert len(res) == 12, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


# ---- the model ----
def _brute(sizes, pairs, arity):
    """the format, read off the issue's wording with sets: per tree (proof nodes per level in visiting order, digests); P_t is empty
    for a tree without pairs"""
    out = {}
    for t in sorted({t for t, _ in pairs}):
        S, w, proof, hashed = {leaf for tt, leaf in pairs if tt == t}, sizes[t], [], 0
        while w > 1:
            parents = sorted({i // arity for i in S})
            proof.append([c for p in parents for c in range(p * arity, p * arity + arity) if c < w and c not in S])
            hashed += len(parents)
            S, w = set(parents), (w + arity - 1) // arity
        out[t] = (proof, hashed)
    return out


def _forests(rng):
    """(sizes, tree_ids, leaf_ids): forests of sizes drawn from SIZES with random pair sets — trees with no pair and with every leaf"""
    for trial in range(24):
        sizes = rng.choice(SIZES, size=int(rng.integers(1, 9))).astype(np.int64)
        tid, lid = [], []
        for t, n in enumerate(sizes):
            mode = int(rng.integers(0, 4))
            if n == 0 or mode == 0:
                continue  # nobody asks
            pos = np.arange(n) if mode == 1 else np.sort(rng.choice(n, int(rng.integers(1, n + 1)), replace=False))
            tid += [t] * len(pos)
            lid += pos.tolist()
        if tid:
            yield sizes, np.array(tid, dtype=np.int64), np.array(lid, dtype=np.int64)


def _numbered_forest(sizes, arity):
    """leaves and tree-major levels whose scalar (tree, level, node) is [tree, level, node, 0]: a proof of them names its nodes"""
    leaves, levels = [], []
    for t, n in enumerate(sizes):
        leaves += [[t, 0, i, 0] for i in range(n)]
        w, l = int(n), 0
        while w > 1:
            w, l = (w + arity - 1) // arity, l + 1
            levels += [[t, l, i, 0] for i in range(w)]
    as_arr = lambda rows: np.array(rows, dtype=np.uint64).reshape(-1, 4)  # noqa: E731
    return as_arr(leaves), as_arr(levels)


def test_model_agrees_with_a_brute_force_set_construction_and_the_bound_holds():
    from poseidon252_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(11)
    for arity in (4, 2):
        bound_fn = getattr(L, "p252_merkle%d_forest_ragged_multiproof_bound" % arity)
        n_forests = 0
        for sizes, tid, lid in _forests(rng):
            n_forests += 1
            leaves, levels = _numbered_forest(sizes, arity)
            offsets = np.concatenate([[0], np.cumsum(sizes)])
            out, proof, po = forest_multiproof_extract(leaves, offsets, levels, tid, lid, arity)
            want = _brute(sizes, list(zip(tid.tolist(), lid.tolist())), arity)
            names = [[t, l, c, 0] for t in sorted(want) for l, level in enumerate(want[t][0]) for c in level]
            assert proof.tolist() == names, (arity, sizes, tid, lid)
            assert out.tolist() == [[t, 0, i, 0] for t, i in zip(tid.tolist(), lid.tolist())]
            lens = np.diff(po.astype(np.int64))
            for t in range(len(sizes)):
                assert lens[t] == (sum(len(x) for x in want[t][0]) if t in want else 0), (arity, sizes, t)
                if sizes[t] <= 1 or (t in want and (tid == t).sum() == sizes[t]):
                    assert lens[t] == 0  # a one-leaf tree, and a tree all of whose leaves are asked for
            po2, hashed = forest_multiproof_counts(sizes, tid, lid, arity)
            assert np.array_equal(po, po2) and hashed == sum(h for _, h in want.values())
            n, T, top, k = int(sizes.sum()), len(sizes), int(sizes.max()), len(tid)
            bound = bound_fn(n, T, top, k)
            assert bound == forest_multiproof_bound(n, T, top, k, arity) >= int(po[-1]), (arity, sizes, k)
        assert n_forests >= 20
        for d in range(0, 6):  # one leaf in each complete tree of a forest of equal complete trees: the bound is reached
            n, T = arity ** d, 5
            sizes = np.full(T, n, dtype=np.int64)
            po, _ = forest_multiproof_counts(sizes, np.arange(T), np.full(T, n // 3), arity)
            assert int(po[-1]) == bound_fn(n * T, T, n, T) == T * d * (arity - 1)
        assert bound_fn(0, 3, 5, 4) == 0 and bound_fn(12, 0, 5, 4) == 0 and bound_fn(12, 3, 5, 0) == 0


@pytest.mark.parametrize("arity", [4, 2])
def test_model_with_the_oracles_digest_gives_the_oracles_roots(oracle_mod, arity):
    tag = E._mtag(arity)
    digest = lambda x: oracle_mod.hash_batch(tag, x, arity, 1)  # noqa: E731
    rng = np.random.default_rng(5 + arity)
    sizes = np.array([5, 17, 1, 64, 0, 65, 21, 2], dtype=np.int64)
    leaves = oracle_mod.fill_random(70 + arity, int(sizes.sum()))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    trees = [E.oracle_tree(tag, leaves[offsets[t]:offsets[t + 1]], arity) if sizes[t] else (None, np.zeros((0, 4), dtype=np.uint64))
             for t in range(len(sizes))]
    levels = np.concatenate([lv for _, lv in trees])
    tid, lid = [], []
    for t in (0, 1, 2, 3, 5, 7):
        pos = np.sort(rng.choice(sizes[t], max(1, sizes[t] // 3), replace=False))
        tid += [t] * len(pos)
        lid += pos.tolist()
    out, proof, po = forest_multiproof_extract(leaves, offsets, levels, tid, lid, arity)
    roots = forest_multiproof_roots(sizes, tid, lid, out, proof, po, arity, digest, reduce=E.reduce_mod_p)
    assert sorted(roots) == [0, 1, 2, 3, 5, 7]
    for t, root in roots.items():
        assert np.array_equal(root, trees[t][0]), (arity, t)
    # a changed proof scalar changes only its own tree's root
    at = int(po[3]) + 1
    assert at < int(po[4])
    changed = proof.copy()
    changed[at, 1] ^= np.uint64(1)
    roots2 = forest_multiproof_roots(sizes, tid, lid, out, changed, po, arity, digest, reduce=E.reduce_mod_p)
    for t in roots:
        assert np.array_equal(roots2[t], roots[t]) == (t != 3), (arity, t)


# ---- the Python mirror ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_validate_before_any_device_call(recorder, arity):
    from poseidon252_amd import Context
    ctx = Context.__new__(Context)  # no device: nothing below may reach one
    ctx._h, ctx.device = None, 0
    tag = np.zeros(4, dtype=np.uint64)
    n, T, top, k, cap = 40, 3, 16, 5, 12
    D = 2 if arity == 4 else 4
    i32, u8 = torch.int32, torch.uint8
    good = dict(d_leaves=_dev(n * 4), d_offsets=_dev(T + 1), d_levels=_dev((n // (arity - 1) + T * D) * 4), d_tree_ids=_dev(k, i32),
                d_leaf_ids=_dev(k), d_leaves_out=_dev(k * 4), d_proof=_dev(cap * 4), d_proof_offsets=_dev(T + 1), d_n_bad=_dev(1, i32),
                d_leaves_in=_dev(k * 4), d_roots=_dev(T * 4), d_ok=_dev(T, u8), d_roots_out=_dev(T * 4), d_n_hashed=_dev(1))

    def extract(a, k=k):
        f = ctx.merkle4_forest_ragged_multiproof_device if arity == 4 else ctx.merkle2_forest_ragged_multiproof_device
        return f(a["d_leaves"], a["d_offsets"], T, top, a["d_levels"], a["d_tree_ids"], a["d_leaf_ids"], k, a["d_leaves_out"], a["d_proof"],
                 a["d_proof_offsets"], d_n_bad=a["d_n_bad"])

    def verify(a, k=k, proof_len=cap):
        f = ctx.merkle4_forest_ragged_multiproof_verify_device if arity == 4 else ctx.merkle2_forest_ragged_multiproof_verify_device
        return f(tag, a["d_offsets"], n, T, top, a["d_tree_ids"], a["d_leaf_ids"], a["d_leaves_in"], k, a["d_proof"], proof_len,
                 a["d_proof_offsets"], a["d_roots"], a["d_ok"], d_roots_out=a["d_roots_out"], d_n_hashed=a["d_n_hashed"], d_n_bad=a["d_n_bad"])
    calls = {extract: ("p252_merkle%d_forest_ragged_multiproof_device_into" % arity,
                       ["d_leaves", "d_offsets", "d_levels", "d_tree_ids", "d_leaf_ids", "d_leaves_out", "d_proof", "d_proof_offsets", "d_n_bad"]),
             verify: ("p252_merkle%d_forest_ragged_multiproof_verify_device_into" % arity,
                      ["d_offsets", "d_tree_ids", "d_leaf_ids", "d_leaves_in", "d_proof", "d_proof_offsets", "d_roots", "d_ok", "d_roots_out",
                       "d_n_hashed", "d_n_bad"])}
    wrong_dtype = {"d_offsets": i32, "d_tree_ids": torch.int64, "d_leaf_ids": i32, "d_proof_offsets": i32, "d_n_bad": torch.int64,
                   "d_n_hashed": i32, "d_ok": i32}
    n_refused = 0
    for call, (symbol, names) in calls.items():
        call(good)
        assert recorder.calls == [symbol]  # the control: all good -> the library is reached, once
        del recorder.calls[:]
        call(dict(good, d_n_bad=None, d_roots_out=None, d_n_hashed=None))  # the optional ones
        assert recorder.calls == [symbol]
        del recorder.calls[:]
        for name in names:
            t = good[name]
            variants = [("is on cpu", torch.zeros_like(t.as_subclass(torch.Tensor))),                     # a host tensor
                        ("holds", t[:max(t.numel() - 1, 0)] if t.numel() > 1 else _dev(0, t.dtype)),       # one element short
                        ("not contiguous", _dev(2 * t.numel(), t.dtype)[::2]),                              # a strided view
                        ("torch tensor", np.zeros(t.numel()))]                                              # no tensor at all
            if name == "d_leaves" or (name == "d_proof" and call is extract):  # (their lengths ARE n_leaves and the capacity)
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
        assert recorder.calls == []
    assert n_refused >= 75
    for call in (extract, verify):
        with pytest.raises(ValueError, match="holds"):  # d_proof_offsets one short of n_trees + 1
            call(dict(good, d_proof_offsets=_dev(T)))
    with pytest.raises(ValueError, match="holds"):  # a proof_len past the tensor
        verify(good, proof_len=cap + 1)
    with pytest.raises(ValueError, match="torch tensor"):  # a proof_len without a proof
        verify(dict(good, d_proof=None), proof_len=1)
    with pytest.raises(ValueError, match="holds"):  # a d_levels below the build's bound
        extract(dict(good, d_levels=_dev((n // (arity - 1) + T * D) * 4 - 4)))
    assert recorder.calls == []
    verify(dict(good, d_proof=None), proof_len=0)  # an empty proof needs no tensor
    extract(dict(good, d_proof=None))              # and a capacity of zero reports the lengths
    assert len(recorder.calls) == 2


def test_conveniences_are_exported_and_refuse_an_outside_pair_before_any_call():
    import poseidon252_amd as P
    assert "forest_ragged_multiproof" in P.__all__ and "forest_ragged_multiproof_verify" in P.__all__
    with pytest.raises(ValueError, match="arity"):
        P.forest_ragged_multiproof(None, torch.zeros((4, 4), dtype=torch.int64), None, 1, 4, None, [0], [0], arity=3)


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("forest_multiproof_refusals", tmp_path_factory.mktemp("forest_multiproof_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "forest_multiproof_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for name, n_args in ARGS.items():
        by = {r[1]: r[2:] for r in table if r[0] == name}
        if name.endswith("_bound"):
            arity = 4 if "merkle4" in name else 2
            assert by["control"][0] == forest_multiproof_bound(12, 3, 5, 4, arity) == (22 if arity == 4 else 12)
            assert by["k=1000"][0] == forest_multiproof_bound(12, 3, 5, 1000, arity) == (22 if arity == 4 else 33)  # (by its second term)
            assert by["k=0"][0] == by["n_leaves=0"][0] == by["n_trees=0"][0] == 0
            continue
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3
        for case in ("k=0", "n_trees=0", "n_leaves=0", "max_leaves=0"):
            assert refused(case, "must be > 0"), case
        assert refused("k=2^32", "2^32") and accepted("k=2^32-1")
        assert refused("max_leaves=2^32", "2^32") and accepted("max_leaves=2^32-1")
        for case in ("proof_len=SIZE_MAX/32+1", "n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2"):
            assert refused(case, "overflow"), case
        assert accepted("proof_len=SIZE_MAX/32") and accepted("proof_len=0,d_proof=NULL") and accepted("max_leaves=1,d_levels=NULL")
        optional = {"d_n_bad", "d_roots_out", "d_n_hashed"}
        nulls = [c[:-5] for c in by if c.endswith("=NULL") and "," not in c and c not in ("ctx=NULL", "tag=NULL")]
        assert len(nulls) == (9 if name.endswith("multiproof_device_into") else 11), nulls
        for buf in nulls:
            assert accepted(buf + "=NULL") if buf in optional else refused(buf + "=NULL", "NULL buffer"), buf
        for case in by:
            if "+" in case and "=" not in case:  # off its alignment
                assert refused(case, "aligned"), case
        if name.endswith("verify_device_into"):
            assert refused("tag=NULL", "NULL buffer")


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_multiproof_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_multiproof_bench")
