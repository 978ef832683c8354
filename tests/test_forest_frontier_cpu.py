"""A forest of append-only Merkle trees kept only as their frontiers (p252_merkle{4,2}_forest_frontier_append_device_into,
_extract_device_into, _bound; csrc/forest_frontier.hip) — what can be checked without a GPU: the numpy model the GPU tests compare the
calls with (testsupport/forestfrontier.py) against full builds by the oracle, for every small tree and append; the symbols declared,
exported and mirrored; the host refusals as a table; the C++ mirror; the unit hashes nothing itself and its kernels use no private
memory; the Python methods validate every buffer before the library is reached."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport import forestfrontier as FF  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_frontier_bound": 1, "p252_merkle2_forest_frontier_bound": 1,
           "p252_merkle4_forest_frontier_append_device_into": 13, "p252_merkle2_forest_frontier_append_device_into": 13,
           "p252_merkle4_forest_frontier_extract_device_into": 14, "p252_merkle2_forest_frontier_extract_device_into": 14}
N_MAX, M_MAX, MAX_LEAVES = 70, 20, 90


def _tag(arity):
    from poseidon252_amd import merkle
    return merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()


# ---- the model against the oracle ----
@pytest.fixture(scope="module")
def builds(oracle_mod):
    """per arity: the leaves, and (root, levels) of the oracle's build of their first n, n = 1 .. N_MAX + M_MAX — computed once"""
    out = {}
    for arity in (4, 2):
        leaves = oracle_mod.fill_random(0xF70 + arity, N_MAX + M_MAX)
        tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
        out[arity] = (leaves, {n: tree(_tag(arity), leaves[:n], want_levels=True)[:2] for n in range(1, N_MAX + M_MAX + 1)})
    return out


def _state(builds, arity, n):
    leaves, built = builds[arity]
    if n == 0:
        return FF.State(arity, MAX_LEAVES)
    root, levels = built[n]
    return FF.State(arity, MAX_LEAVES, n, FF.frontier_of(leaves[:n], levels, n, arity, MAX_LEAVES), root)


@pytest.mark.parametrize("arity", [4, 2])
def test_model_append_equals_the_frontier_of_the_larger_build(oracle_mod, builds, arity):
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    for n in range(N_MAX + 1):
        old = _state(builds, arity, n)
        if n:
            assert np.array_equal(FF.root_of(old, digest), built[n][0]), n  # the chain of partly filled nodes
        for m in range(M_MAX + 1):
            new, hashed = FF.append(old, leaves[n:n + m], digest)
            want = _state(builds, arity, n + m)
            assert new.n == n + m and np.array_equal(new.rows, want.rows) and np.array_equal(new.root, want.root), (arity, n, m)
            assert hashed == FF.n_hashed(n, m, arity), (arity, n, m)
            # the digests computed = the nodes of the larger build that the smaller one does not hold with the same value
            if m:
                lv_old, lv_new = (built[n][1] if n else np.zeros((0, 4), np.uint64)), (built[n + m][1] if n + m > 1 else np.zeros((0, 4), np.uint64))
                s_old, s_new = TS.level_starts(n, arity), TS.level_starts(n + m, arity)
                differ = 0
                for l in range(1, len(s_new)):
                    a = lv_new[s_new[l - 1]:s_new[l]]
                    b = lv_old[s_old[l - 1]:s_old[l]] if l < len(s_old) else lv_old[:0]
                    same = (a[:b.shape[0]] == b[:a.shape[0]]).all(axis=1).sum()
                    differ += a.shape[0] - int(same)
                assert differ == hashed, (arity, n, m)
    # slots past the digit are zero, row D is used by a full tree only
    full = _state(builds, arity, arity ** 3)
    assert full.rows[3, 0].any() and not full.rows[:3].any() and not full.rows[3, 1:].any() and not full.rows[4:].any()


def test_model_shapes():
    assert [FF.bound(n, 4) for n in (0, 1, 2, 4, 5, 16, 17)] == [0, 3, 6, 6, 9, 9, 12]
    assert [FF.bound(n, 2) for n in (0, 1, 2, 3, 4, 5)] == [0, 1, 2, 3, 3, 4]
    assert FF.n_hashed(5, 0, 4) == 0 and FF.n_hashed(0, 1, 4) == 0 and FF.n_hashed(4, 1, 4) == 2 and FF.n_hashed(3, 1, 4) == 1
    assert FF.n_hashed(0, 5, 2) == 3 + 2 + 1 and FF.n_hashed(7, 1, 2) == 1 + 1 + 1


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    raw, header = check_abi_symbols(SYMBOLS)
    assert "forest_frontier" in raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    # no new name that the refusal table of the `_device(` symbols would have to hold: that table stays as it is
    assert not any("frontier" in s for s in re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))


def test_bound_equals_the_model():
    from poseidon252_amd import _lib
    L = _lib.lib()
    for arity, f in ((4, L.p252_merkle4_forest_frontier_bound), (2, L.p252_merkle2_forest_frontier_bound)):
        for n in list(range(0, 70)) + [255, 256, 257, 4 ** 12, 4 ** 12 + 1, 2 ** 32 - 1, 2 ** 32]:
            assert int(f(n)) == FF.bound(n, arity), (arity, n)


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("frontier_refusal_table", tmp_path_factory.mktemp("frontier_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "frontier_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_frontier_append_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and by["n_trees=0"] == (0, "") and by["n_trees=0,max_leaves=0"] == (0, "")
        assert refused("max_leaves=0", "max_leaves") and accepted("max_leaves=1") and accepted("max_leaves=SIZE_MAX")
        assert refused("n_add=2^32", "2^32") and refused("n_add=SIZE_MAX", "2^32") and accepted("n_add=2^32-1")
        assert accepted("n_add=0") and accepted("n_add=0,d_add=NULL") and accepted("n_add=0,d_roots=d_add")
        for case in ("n_trees=SIZE_MAX/8/66+1", "n_trees=SIZE_MAX/64/bound+1", "n_trees*n_add>SIZE_MAX/2"):
            assert refused(case, "size overflow"), case
        for buf in ("tag", "d_counts", "d_frontier", "d_roots", "d_add", "d_add_offsets"):
            assert refused(buf + "=NULL", "NULL buffer"), buf
        assert accepted("d_n_bad=NULL") and accepted("d_n_hashed=NULL")
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 7 and all(refused(c, "aligned") for c in misaligned)
        for o in ("d_counts", "d_frontier", "d_roots", "d_n_bad", "d_n_hashed"):  # the state against both inputs, on both sides of their ends
            for i in ("d_add", "d_add_offsets"):
                assert refused("%s=%s+last" % (o, i), "%s overlaps %s" % (o, i)), (o, i)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
        assert refused("d_frontier=d_add-bytes+16", "overlaps") and accepted("d_frontier=d_add-bytes")

        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_frontier_extract_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")
        assert by["ctx=NULL"][0] == -3 and by["n_trees=0"] == (0, "")
        assert refused("max_leaves_forest=0", "max_leaves") and refused("max_leaves=max_leaves_forest-1", "max_leaves")
        assert accepted("max_leaves=max_leaves_forest") and accepted("max_leaves_forest=1,d_levels=NULL")
        assert refused("n_leaves=SIZE_MAX/64+1", "size overflow") and refused("n_trees=SIZE_MAX/8/66+1", "size overflow")
        for buf in ("d_leaves", "d_offsets", "d_levels", "d_roots_forest", "d_counts", "d_frontier", "d_roots"):
            assert refused(buf + "=NULL", "NULL buffer"), buf
        assert accepted("d_n_bad=NULL")
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 8 and all(refused(c, "aligned") for c in misaligned)
        for o in ("d_counts", "d_frontier", "d_roots", "d_n_bad"):
            for i in ("d_leaves", "d_offsets", "d_levels", "d_roots_forest"):
                assert refused("%s=%s+last" % (o, i), "%s overlaps %s" % (o, i)), (o, i)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
        # the bound, as the model has it
        rows = {r[1]: r[2] for r in table if r[0] == "p252_merkle%d_forest_frontier_bound" % arity}
        assert rows["max_leaves=0"] == 0 and rows["max_leaves=1"] == arity - 1 and rows["max_leaves=0x11"] == FF.bound(17, arity)
        assert rows["max_leaves=0x1000001"] == FF.bound(2 ** 24 + 1, arity)


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_frontier.hip", os.path.join(CSRC, "_gen", "forest_frontier_test.s"))


def test_kernels_use_no_private_memory(compiled):
    res, isa = compiled
    assert all("k_ff_" in n for n in res), sorted(res)
    assert sorted(re.search(r"k_ff_[a-z_]+", n).group(0) for n in res) == ["k_ff_extract", "k_ff_finish", "k_ff_records", "k_ff_refused", "k_ff_sizes"]
    for name, v in res.items():  # bookkeeping and data movement: no private memory, a quarter of the register file at the most
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_the_unit_hashes_nothing_itself():
    from poseidon252_amd import build as b
    import edgecases
    assert "forest_frontier.hip" in b.SOURCES and "forest_frontier.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_frontier.hip")).read()
    for word in ("hades_permute", "node_digest_coop", "asm"):
        assert word not in src, word
    assert "launch_multiproof_digest_list" in src and "launch_forest_ragged_index" in src
    # the scans over the trees and the search of a node's tree are the stored append's (blockops.hpp's primitives), through its
    # launchers: no fresh copy of a scan loop or of a search here, and the neighbours' kernels through their launchers only
    assert "forest_append_scan_sum_rule" in src and "forest_append_scan_dirty_lists" in src
    assert "for (unsigned off = 1; off <" not in src and "while (lo < hi)" not in src and "__shared__" not in src
    assert not re.search(r"\bk_(mp|fr|fa)_\w+\s*[(<]", re.sub(r"//[^\n]*", "", src))
    assert set(edgecases.hashing_kernels()) <= set(edgecases.named_kernels())
    assert not any("k_ff_" in k for k in edgecases.hashing_kernels())


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32 = torch.int32
    n_trees, max_leaves, n_add = 3, 100, 8
    stride = FF.bound(max_leaves, arity)
    args = dict(d_counts=dev(), d_frontier=dev(n=n_trees * stride * 4), d_roots=dev(), d_add=dev(n=n_add * 4), d_add_offsets=dev(),
                d_n_bad=dev(i32), d_n_hashed=dev())
    method = ctx.merkle4_forest_frontier_append_device if arity == 4 else ctx.merkle2_forest_frontier_append_device

    def call(a):
        return method(tag, a["d_counts"], a["d_frontier"], a["d_roots"], n_trees, max_leaves, a["d_add"], a["d_add_offsets"], a["d_n_bad"], a["d_n_hashed"])
    symbol = "p252_merkle%d_forest_frontier_append_device_into" % arity
    call(args)
    assert recorder.calls == [symbol]  # the control: the library is reached, once, under this arity's symbol
    del recorder.calls[:]
    n_refused = 0
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call(bad)
        n_refused += 1
    assert n_refused == 7 and recorder.calls == []
    for name, short in (("d_counts", dev(n=n_trees - 1)), ("d_frontier", dev(n=n_trees * stride * 4 - 1)), ("d_roots", dev(n=n_trees * 4 - 1)),
                        ("d_add_offsets", dev(n=n_trees))):
        with pytest.raises(ValueError, match=name + " holds"):
            call(dict(args, **{name: short}))
    for name in ("d_counts", "d_add_offsets", "d_n_hashed"):
        with pytest.raises(ValueError, match=name + " needs 8-byte elements"):
            call(dict(args, **{name: dev(i32)}))
    assert recorder.calls == []
    assert "arity" not in __import__("inspect").signature(method).parameters
    # the extraction
    n_leaves, max_forest = 16, 9
    depth = TS.depth(max_forest, arity)
    ex = dict(d_leaves=dev(n=n_leaves * 4), d_offsets=dev(), d_levels=dev(n=(n_leaves // (arity - 1) + n_trees * depth) * 4), d_roots_forest=dev(),
              d_counts=dev(), d_frontier=dev(n=n_trees * stride * 4), d_roots=dev(), d_n_bad=dev(i32))
    extract = ctx.merkle4_forest_frontier_extract_device if arity == 4 else ctx.merkle2_forest_frontier_extract_device

    def call_ex(a):
        return extract(a["d_leaves"], a["d_offsets"], n_trees, max_forest, a["d_levels"], a["d_roots_forest"], max_leaves, a["d_counts"], a["d_frontier"],
                       a["d_roots"], a["d_n_bad"])
    call_ex(ex)
    assert recorder.calls == ["p252_merkle%d_forest_frontier_extract_device_into" % arity]
    del recorder.calls[:]
    assert sum(1 for _ in with_cpu_tensor(ex)) == 8
    for where, bad in with_cpu_tensor(ex):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call_ex(bad)
    with pytest.raises(ValueError, match="d_levels holds"):
        call_ex(dict(ex, d_levels=dev(n=(n_leaves // (arity - 1) + n_trees * depth) * 4 - 1)))
    assert recorder.calls == [] and "arity" not in __import__("inspect").signature(extract).parameters
    # the sizes the C calls receive
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name in (symbol, "p252_merkle%d_forest_frontier_extract_device_into" % arity):
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    call(args)
    call(dict(args, d_add=None, d_n_bad=None, d_n_hashed=None))
    call_ex(ex)
    a, b, c = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert a[2:] == (ptr(args["d_counts"]), ptr(args["d_frontier"]), ptr(args["d_roots"]), n_trees, max_leaves, ptr(args["d_add"]), n_add,
                     ptr(args["d_add_offsets"]), ptr(args["d_n_bad"]), ptr(args["d_n_hashed"]), 0)
    assert b[7:] == (None, 0, ptr(args["d_add_offsets"]), None, None, 0)
    assert c[1:] == (ptr(ex["d_leaves"]), n_leaves, ptr(ex["d_offsets"]), n_trees, max_forest, ptr(ex["d_levels"]), ptr(ex["d_roots_forest"]), max_leaves,
                     ptr(ex["d_counts"]), ptr(ex["d_frontier"]), ptr(ex["d_roots"]), ptr(ex["d_n_bad"]), 0)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_frontier_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_frontier_bench")
