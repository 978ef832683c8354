"""A forest of trees of different sizes rolled back, and forward again, in one call
(p252_merkle{4,2}_forest_ragged_resize_device_into; csrc/forest_append.hip) — what can be checked without a GPU: the numpy model the
GPU tests compare the call with agrees with a brute-force construction of both trees and with trees hashed by the big-int model of
the permutation; the two entry points are declared, exported and mirrored in the Rust FFI under ABI 9, under a name the refusal table
of the `_device(` symbols does not catch; forest_append.hip still compiles for gfx950 within its resource targets; the host
refusals, as a table of their own; the Python methods validate every buffer before the library is reached and hand the C call the
right sizes."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport.forestappend import KEEP_ALL, forest_append_model, forest_resize_model, model_leaves  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import (ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols,  # noqa: E402
                             refusal_table)
from testsupport.treeshape import level_widths  # noqa: E402

SYMBOLS = ("p252_merkle4_forest_ragged_resize_device_into", "p252_merkle2_forest_ragged_resize_device_into")
N_ARGS = 23


# ---- the model ----
def _brute_levels(leaves, arity):
    """levels 1.. of a tree of the given leaves (any hashable values), each node the tuple of its children (None: a missing child)"""
    cur, out = list(leaves), []
    while len(cur) > 1:
        cur = [tuple(cur[j * arity + c] if j * arity + c < len(cur) else None for c in range(arity)) for j in range((len(cur) + arity - 1) // arity)]
        out.append(cur)
    return out


def _single(n, k, m, arity):
    return forest_resize_model([0, n], n, max(n, 1), [k], [0, m], m, max(n + m, 1), arity)


def test_model_agrees_with_a_brute_force_construction_of_both_trees():
    for arity in (4, 2):
        for n in range(40):
            old = _brute_levels([("old", i) for i in range(n)], arity)
            for k in range(n + 1):
                for m in range(22):
                    new = _brute_levels([("old", i) for i in range(k)] + [("add", i) for i in range(m)], arity)
                    M = _single(n, k, m, arity)
                    assert M["n_old"] == [n] and M["k"] == [k] and M["m"] == [m] and M["offsets_new"].tolist() == [0, k + m]
                    assert M["n_bad"] == (1 if k + m == 0 else 0)
                    assert M["leaf_src"].tolist() == list(range(k)) + [-1 - i for i in range(m)]
                    unchanged = k == n and m == 0
                    # every slot of the new tree: clean iff the same node sits at the same (level, index) of the old tree iff the rule
                    slot, want_dirty, old_start = 0, {}, 0
                    assert len(M["node_src"]) == sum(len(lv) for lv in new) and len(M["node_id"]) == len(M["node_src"])
                    for l, lv in enumerate(new, 1):
                        for j, node in enumerate(lv):
                            clean = l <= len(old) and j < len(old[l - 1]) and old[l - 1][j] == node
                            assert M["node_id"][slot] == (0, l, j)
                            assert M["node_src"][slot] == (old_start + j if clean else -1), (arity, n, k, m, l, j)
                            assert clean == (unchanged or j < k // arity ** l), (arity, n, k, m, l, j)
                            if not clean:
                                want_dirty.setdefault(l, []).append((0, j))
                            slot += 1
                        old_start += len(old[l - 1]) if l <= len(old) else 0
                    assert M["dirty"] == want_dirty
                    per_level = [0 if unchanged else -(-(k + m) // arity ** l) - k // arity ** l for l in range(1, len(new) + 1)]
                    assert [len(want_dirty.get(l, [])) for l in range(1, len(new) + 1)] == per_level, (arity, n, k, m)
                    assert M["n_hashed"] == sum(per_level)
                    assert all(d <= m // arity ** l + 2 for l, d in enumerate(per_level, 1))  # the bound of the dirty lists
                    if m == 0:
                        assert all(d <= 1 for d in per_level), (arity, n, k)


def test_keep_none_is_the_append_model():
    off, n_leaves, max_leaves = [5, 8, 8, 12, 30, 31], 40, 10
    aoff, n_add = [0, 2, 5, 4, 5, 20, 20, 26], 26
    A = forest_append_model(off, n_leaves, max_leaves, aoff, n_add, 12, 4)
    for keep in (None, [KEEP_ALL] * 7, [-1] * 7, [100] * 7):
        R = forest_resize_model(off, n_leaves, max_leaves, keep, aoff, n_add, 12, 4)
        assert R["k"] == A["n_old"]
        for key, want in A.items():
            assert np.array_equal(R[key], want) if isinstance(want, np.ndarray) else R[key] == want, key


def test_model_of_a_forest_cuts_refusals_dropped_and_new_trees():
    # old forest of 8 trees: offsets start at 5; tree 1 empty, tree 3 longer than max_leaves (bad: its leaves are dropped)
    off, n_leaves, max_leaves = [5, 8, 8, 12, 30, 31, 39, 45, 50], 60, 10
    # the new forest has 9 trees: tree 8 is new (the same old forest with its trailing trees dropped: further down)
    #        tree 0    1 (empty)  2          3 (bad)  4         5            6          7           8 (new)
    keep = [0,        1,         KEEP_ALL,  2,       9,        3,           1,         6,          5]
    # appends: +2 to the tree cut to nothing; +0; +1; +1 to the bad tree; +0; 3 + 8 > max_leaves_new (refused: still cut to 3); decreasing
    # (refused: still cut to 1); +0 (keep 6 > n = 5: whole); +4 to the new tree
    aoff, n_add = [0, 2, 2, 3, 4, 4, 12, 11, 11, 15], 15
    M = forest_resize_model(off, n_leaves, max_leaves, keep, aoff, n_add, 10, 4)
    assert M["n_old"] == [3, 0, 4, 0, 1, 8, 6, 5, 0]
    assert M["k"] == [0, 0, 4, 0, 1, 3, 1, 5, 0]
    assert M["m"] == [2, 0, 1, 1, 0, 0, 0, 0, 4] and M["refused"] == [False, False, False, False, False, True, True, False, False]
    assert M["n_new"] == [2, 0, 5, 1, 1, 3, 1, 5, 4] and M["offsets_new"].tolist() == [0, 2, 2, 7, 8, 9, 12, 13, 18, 22]
    assert M["n_bad"] == 3  # two refused, one empty
    leaves, add = np.arange(60 * 4).reshape(60, 4), 1000 + np.arange(15 * 4).reshape(15, 4)
    got = model_leaves(M, leaves, add)
    assert np.array_equal(got[0:2], add[0:2]) and np.array_equal(got[2:7], np.concatenate([leaves[8:12], add[2:3]]))
    assert np.array_equal(got[7:8], add[3:4]) and np.array_equal(got[8:9], leaves[30:31]) and np.array_equal(got[9:12], leaves[31:34])
    assert np.array_equal(got[12:13], leaves[39:40]) and np.array_equal(got[13:18], leaves[45:50]) and np.array_equal(got[18:22], add[11:15])
    # digests: tree 0 (0 + 2) 1; tree 2 (4 + 1) 2 - 1 + 1 = 2; trees 3, 4 (one leaf) 0; tree 5 (8 cut to 3) 1; tree 6 (cut to 1) 0;
    # tree 7 unchanged 0; tree 8 (0 + 4) 1
    assert M["n_hashed"] == 5 and M["dirty"] == {1: [(0, 0), (2, 1), (5, 0), (8, 0)], 2: [(2, 0)]}
    # trailing trees dropped, nothing else: the three survivors unchanged
    M = forest_resize_model(off, n_leaves, max_leaves, None, [0, 0, 0, 0], 0, 10, 2)
    assert M["n_new"] == [3, 0, 4] and M["n_hashed"] == 0 and M["n_bad"] == 1 and (M["node_src"] >= 0).all()
    # a cut to a whole power of the arity: the root itself is a clean node
    M = forest_resize_model([0, 21], 21, 21, [16], [0, 0], 0, 21, 4)
    assert M["n_hashed"] == 0 and M["node_src"].tolist() == [0, 1, 2, 3, 6]
    M = forest_resize_model([0, 21], 21, 21, [16], [0, 0], 0, 21, 2)
    assert M["n_hashed"] == 0 and len(M["node_src"]) == 15


def _pymodel_levels(leaves, arity, tag):
    import pymodel
    cur, out = list(leaves), []
    while len(cur) > 1:
        cur = [pymodel.sponge(tag, [cur[j * arity + c] if j * arity + c < len(cur) else 0 for c in range(arity)], 1)[0]
               for j in range((len(cur) + arity - 1) // arity)]
        out += cur
    return out


@pytest.mark.parametrize("arity,n,k,m", [(4, 9, 5, 0), (4, 21, 16, 0), (4, 6, 1, 0), (4, 7, 4, 3), (2, 7, 5, 0), (2, 9, 4, 2), (2, 6, 3, 4)])
def test_model_against_trees_hashed_by_the_big_int_model(oracle_mod, arity, n, k, m):
    """the clean slots of the resized tree hold the old tree's values, the dirty ones do not; one root of each shape is the oracle's"""
    import pymodel
    from poseidon252_amd import merkle
    R = 1 << 256
    to_int = lambda a: [int.from_bytes(np.ascontiguousarray(s).tobytes(), "little") * pow(R, -1, pymodel.P) % pymodel.P for s in a]  # noqa: E731
    tag_limbs = merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()
    tag = to_int([tag_limbs])[0]
    limbs = oracle_mod.fill_random(0xC99 + n, n + m)
    new_limbs = np.concatenate([limbs[:k], limbs[n:]])
    vals, new_vals = to_int(limbs), to_int(new_limbs)
    old, new = _pymodel_levels(vals[:n], arity, tag), _pymodel_levels(new_vals, arity, tag)
    M = _single(n, k, m, arity)
    assert len(new) == len(M["node_src"])
    w_old = level_widths(n, arity)
    for slot, src in enumerate(M["node_src"].tolist()):
        t, l, j = M["node_id"][slot]
        if src >= 0:
            assert new[slot] == old[src], (slot, src)
        elif l <= len(w_old) and j < w_old[l - 1]:  # a cut or a new leaf below it: not the value the old tree had at (l, j)
            assert new[slot] != old[sum(w_old[:l - 1]) + j], slot
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    root = tree(tag_limbs, new_limbs)[0]
    assert (new[-1] if new else new_vals[0]) == to_int([root])[0]


# ---- the symbols ----
def test_two_symbols_declared_exported_and_in_sys_rs():
    _, header = check_abi_symbols(dict.fromkeys(SYMBOLS, N_ARGS))
    args = lambda name: re.search(r"\bint %s\s*\((.*?)\);" % name, header, flags=re.S).group(1)  # noqa: E731
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    for name in SYMBOLS:  # the append call's arguments with d_keep after d_levels
        app = args(name.replace("resize", "append"))
        assert norm(args(name)) == norm(app.replace("const void* d_levels,", "const void* d_levels, const void* d_keep,")), name
    # no new name that the refusal table of the `_device(` symbols would have to hold: that table stays as it is
    declared = set(re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))
    table = {line.split("\t")[0] for line in open(os.path.join(ROOT, "tests", "golden", "api_refusals.txt")).read().splitlines()}
    assert declared == table and not any("resize" in s for s in declared)


# ---- the kernels ----
def test_kernels_meet_resource_targets_and_the_unit_is_one():
    res, isa = kernel_resources("forest_append.hip", os.path.join(CSRC, "_gen", "forest_resize_test.s"))
    assert len(res) >= 8 and all("k_fa_" in n for n in res), sorted(res)
    for name, v in res.items():  # data movement and bookkeeping: no private memory, a quarter of the register file at the most
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa
    # generalised, not copied: one launcher, one kernel of each name, and still no hashing in the unit
    src = open(os.path.join(CSRC, "forest_append.hip")).read()
    kernels = re.findall(r"__global__ void (?:__launch_bounds__\(\w+\) )?(k_fa_\w+)\(", src)
    assert sorted(kernels) == sorted(set(kernels)) and len(kernels) == 9, kernels
    assert len(re.findall(r"^hipError_t launch_\w+\(", src, flags=re.M)) == 1
    for word in ("hades_permute", "node_digest_coop", "asm"):
        assert word not in src, word
    api = open(os.path.join(CSRC, "api.cpp")).read() + open(os.path.join(CSRC, "api_forest.cpp")).read()  # the host ABI, both files
    assert api.count("launch_forest_append(") == 1 and api.count("forest_append_plan(") == 1  # both entry points, one path


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("resize_refusals", tmp_path_factory.mktemp("resize_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "resize_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for sym in SYMBOLS:
        by = {r[1]: r[2:] for r in table if r[0] == sym}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and by["n_trees_new=0"] == (0, "")
        assert refused("max_leaves_new=max_leaves-1", "max_leaves_new") and accepted("max_leaves_new=max_leaves")
        assert accepted("n_trees_new=n_trees-1") and accepted("n_trees_new=n_trees") and accepted("n_trees_new=1")  # fewer trees: the difference from the append
        assert accepted("d_keep=NULL") and accepted("d_keep=NULL,n_trees_new=n_trees-1") and accepted("n_add=0,d_add=NULL,d_keep=NULL")
        assert refused("leaves_cap=n_leaves+n_add-1", "leaves_cap") and accepted("leaves_cap=n_leaves+n_add+7")
        assert refused("levels_cap=need-1", "levels_cap") and accepted("levels_cap=need+1")
        assert refused("max_leaves=1,max_leaves_new=2,d_levels=d_levels_new=NULL", "NULL") and accepted("max_leaves=1,d_levels=NULL")
        assert accepted("max_leaves=max_leaves_new=1,d_levels=d_levels_new=NULL") and accepted("n_add=0,d_add=NULL")
        assert accepted("n_trees=0,d_leaves=d_offsets=d_levels=NULL,n_leaves=0")
        for case in ("n_leaves=SIZE_MAX/64+1", "n_add=SIZE_MAX", "leaves_cap=SIZE_MAX/64+1", "n_trees_new=SIZE_MAX/8/66+1"):
            assert refused(case, "size overflow"), case
        for buf in ("d_leaves", "d_offsets", "d_levels", "d_add", "d_add_offsets", "d_leaves_new", "d_offsets_new", "d_levels_new", "d_roots"):
            assert refused(buf + "=NULL", "NULL buffer"), buf
        for buf in ("d_n_bad", "d_n_hashed"):
            assert accepted(buf + "=NULL"), buf
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 12 and "d_keep+4" in misaligned and all(refused(c, "aligned") for c in misaligned)
        outs = ("d_leaves_new", "d_offsets_new", "d_levels_new", "d_roots", "d_n_bad", "d_n_hashed")
        ins = ("d_leaves", "d_offsets", "d_levels", "d_add", "d_add_offsets", "d_keep")
        for o in outs:  # every output against every input, on both sides of the input's end
            for i in ins:
                assert refused("%s=%s+last" % (o, i), "%s overlaps %s" % (o, i)), (o, i)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
        assert refused("d_roots=d_add-16", "overlaps") and accepted("d_roots=d_add-4*32")


def test_the_append_entry_points_still_refuse_fewer_trees():
    """the shared validation kept the append's own rule (its table, tests/golden/append_refusals.txt, is compared by its own test)"""
    golden = open(os.path.join(ROOT, "tests", "golden", "append_refusals.txt")).read()
    assert "n_trees_new=n_trees-1\t-3\tmerkle_forest_ragged_append: n_trees_new must be >= n_trees" in golden


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32 = torch.int32
    n_leaves, n_add, n_trees, n_trees_new, max_leaves, max_new, cap = 16, 8, 3, 2, 9, 12, 30
    D = {4: 2, 2: 4}[arity]
    levels_cap = 24 // (arity - 1) + n_trees_new * D + 5
    args = dict(d_leaves=dev(n=n_leaves * 4), d_offsets=dev(), d_levels=dev(n=256), d_keep=dev(), d_add=dev(n=n_add * 4), d_add_offsets=dev(),
                d_leaves_new=dev(n=cap * 4), d_offsets_new=dev(), d_levels_new=dev(n=levels_cap * 4), d_roots=dev(), d_n_bad=dev(i32), d_n_hashed=dev())
    method = ctx.merkle4_forest_ragged_resize_device if arity == 4 else ctx.merkle2_forest_ragged_resize_device

    def call(a):
        return method(tag, a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_keep"], a["d_add"], a["d_add_offsets"], n_trees_new,
                      max_new, a["d_leaves_new"], a["d_offsets_new"], a["d_levels_new"], a["d_roots"], a["d_n_bad"], a["d_n_hashed"])
    symbol = "p252_merkle%d_forest_ragged_resize_device_into" % arity
    call(args)
    assert recorder.calls == [symbol]  # the control: the library is reached, once, under this arity's symbol
    del recorder.calls[:]
    n_refused = 0
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call(bad)
        assert recorder.calls == [], where
        n_refused += 1
    assert n_refused == 12
    for name, short in (("d_offsets", dev(n=n_trees)), ("d_keep", dev(n=n_trees_new - 1)), ("d_add_offsets", dev(n=n_trees_new)),
                        ("d_offsets_new", dev(n=n_trees_new)), ("d_leaves_new", dev(n=(n_leaves + n_add) * 4 - 1)),
                        ("d_levels_new", dev(n=(24 // (arity - 1) + n_trees_new * D) * 4 - 1)), ("d_roots", dev(n=n_trees_new * 4 - 1)),
                        ("d_levels", dev(n=(16 // (arity - 1) + n_trees * D) * 4 - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call(dict(args, **{name: short}))
    for name in ("d_offsets", "d_keep", "d_add_offsets", "d_offsets_new", "d_n_hashed"):
        with pytest.raises(ValueError, match=name + " needs 8-byte elements"):
            call(dict(args, **{name: dev(i32)}))
    assert recorder.calls == []
    assert "arity" not in __import__("inspect").signature(method).parameters
    # the sizes the C call receives
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name == symbol:
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    call(args)
    call(dict(args, d_keep=None, d_add=None, d_n_bad=None, d_n_hashed=None))
    a, b = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert a[2:] == (ptr(args["d_leaves"]), n_leaves, ptr(args["d_offsets"]), n_trees, max_leaves, ptr(args["d_levels"]), ptr(args["d_keep"]),
                     ptr(args["d_add"]), n_add, ptr(args["d_add_offsets"]), n_trees_new, max_new, ptr(args["d_leaves_new"]), cap,
                     ptr(args["d_offsets_new"]), ptr(args["d_levels_new"]), levels_cap, ptr(args["d_roots"]), ptr(args["d_n_bad"]),
                     ptr(args["d_n_hashed"]), 0)
    assert len(b) == N_ARGS and b[8:11] == (None, None, 0) and b[-4:] == (ptr(args["d_roots"]), None, None, 0)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_resize_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_resize_bench", options=("--quick", "--append-only"))
