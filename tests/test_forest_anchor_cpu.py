"""Roots and openings of a grown forest against its EARLIER roots (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into;
csrc/forest_anchor.hip) — what can be checked without a GPU: the numpy model the GPU tests compare the call with
(testsupport/forestanchor.py), which reads the GROWN tree's build only, against the oracle's rebuilds of the first c leaves for every
count and every leaf of small trees; the symbols declared, exported and mirrored; the host refusals as a table; the C++ mirror; the
kernels' resources; the Python methods validate every buffer before the library is reached."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport import forestanchor as FA  # noqa: E402
from testsupport import forestconsistency as FC  # noqa: E402
from testsupport import forestfrontier as FF  # noqa: E402
from testsupport import forestwitness as FW  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_ragged_anchor_openings_device_into": 24, "p252_merkle2_forest_ragged_anchor_openings_device_into": 24}
MAX_LEAVES = {4: 1024, 2: 128}  # the stride exceeds every depth


def sizes_of(arity):
    """trees of 1, 2, A, A + 1, A^2 - 1, A^2, A^2 + 1, 37 and (arity 4) 70 leaves"""
    a = arity
    return [1, 2, a, a + 1, a * a - 1, a * a, a * a + 1, 37] + ([70] if a == 4 else [])


def _tag(arity):
    from poseidon252_amd import merkle
    return merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()


def _tree(oracle_mod, arity):
    return oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree


# ---- the model against the oracle's rebuilds ----
@pytest.fixture(scope="module")
def builds(oracle_mod):
    """per arity: the leaves, and (root, levels) of the oracle's build of their first n, n = 1 .. the largest tree — computed once"""
    out = {}
    for arity in (4, 2):
        top = max(sizes_of(arity))
        leaves = oracle_mod.fill_random(0xA70 + arity, top)
        out[arity] = (leaves, {n: _tree(oracle_mod, arity)(_tag(arity), leaves[:n], want_levels=True)[:2] for n in range(1, top + 1)})
    return out


@pytest.mark.parametrize("arity", [4, 2])
def test_model_equals_the_truncated_rebuild_for_every_count_and_leaf(oracle_mod, builds, arity):
    """every tree size n of the list, every 1 <= c <= n, every i < c: out of the build of n leaves alone, the model's root is the root of
    the rebuild of the first c leaves, its opening of leaf i the opening cut out of that rebuild, its digest count the consistency
    model's old_digests(c), and no opening holds more than one partial node"""
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES[arity], arity)
    n_openings, with_partial, no_digest = 0, 0, 0
    for n in sizes_of(arity):
        grown_levels = built[n][1]
        for c in range(1, n + 1):
            P, hashed = FA.partial_nodes(leaves[:n], grown_levels, n, c, arity, digest)
            assert hashed == FC.old_digests(c, arity) == FA.old_digests(c, arity) == len(P), (arity, n, c)
            no_digest += hashed == 0
            want_root = FF.reduce_leaf(leaves[0]) if c == 1 else built[c][0]
            assert np.array_equal(FA.root_of(leaves[:n], grown_levels, n, c, arity, digest, partial=P), want_root), (arity, n, c)
            for i in range(c):
                got, used = FA.opening_of(leaves[:n], grown_levels, n, c, i, arity, D, digest, partial=P)
                assert got == FW.opening_of(leaves[:c], built[c][1], c, i, arity, D), (arity, n, c, i)
                assert used <= 1 and got.depth == TS.depth(c, arity), (arity, n, c, i)
                n_openings += 1
                with_partial += used
    assert n_openings == sum(n * (n + 1) // 2 for n in sizes_of(arity)) and with_partial > n_openings // 4 and no_digest >= 10
    # the bad ones
    n = 37
    for c, i in ((0, 0), (n + 1, 0), (5, 5), (5, n)):
        got, used = FA.opening_of(leaves[:n], built[n][1], n, c, i, arity, D, digest)
        assert got.bad() and used == 0 and not got.leaf.any() and not got.siblings.any() and not got.positions.any()
    # the digest count, by hand: A + 1 = 1 * A^0 + 1 * A^1 -> levels 1 and 2; A^2 + A: from level 2 up; a power of the arity: none
    assert FA.old_digests(arity + 1, arity) == 2 and FA.old_digests(arity ** 2 + arity, arity) == 2 and FA.old_digests(arity ** 3, arity) == 0
    assert FA.old_digests(1, arity) == 0 and FA.old_digests(3, arity) == (1 if arity == 4 else 2)


@pytest.mark.parametrize("arity", [4, 2])
def test_model_root_equals_the_frontiers_root(oracle_mod, builds, arity):
    """the root at c out of the grown tree's build is the root a frontier fed the same c leaves recomputes from its rows alone"""
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    n = max(sizes_of(arity))
    state = FF.State(arity, MAX_LEAVES[arity])
    for c in range(1, n + 1):
        state, _ = FF.append(state, leaves[c - 1:c], digest)
        assert np.array_equal(FA.root_of(leaves[:n], built[n][1], n, c, arity, digest), FF.root_of(state, digest)), (arity, c)


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    raw, header = check_abi_symbols(SYMBOLS)
    listed = raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    assert "_forest_ragged_anchor_openings_device_into" in listed
    assert not any("anchor" in s for s in re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))
    # the header says what the layout is for
    doc = raw[raw.index("/* ---- anchors:"):raw.index("int p252_merkle4_forest_ragged_anchor_openings_device_into")]
    assert "d_tree_ids := d_anchor_ids" in doc and "d_roots := d_anchor_roots" in doc and "n_trees := m" in doc and "path_ragged_device" in doc
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("anchor_refusal_table", tmp_path_factory.mktemp("anchor_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "anchor_refusals")


INS = ("d_leaves", "d_offsets", "d_levels", "d_anchor_tree_ids", "d_anchor_counts", "d_anchor_ids", "d_leaf_ids")
OUTS = ("d_anchor_roots", "d_anchor_depths", "d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_n_bad_anchors", "d_n_bad", "d_n_hashed")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_ragged_anchor_openings_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and by["m=0,k=0"] == (0, "") and by["m=0,k=0,all=NULL,max_leaves=0"] == (0, "")
        assert refused("tag=NULL", "NULL buffer")
        # the roots alone, and openings under no anchor
        assert accepted("k=0") and accepted("k=0,openings=NULL") and refused("k=0,d_anchor_roots=NULL", "NULL buffer")
        assert accepted("m=0") and accepted("m=0,anchors=NULL") and refused("m=0,d_leaves_out=NULL", "NULL buffer")
        for case in ("max_leaves=0", "n_trees=0", "n_leaves=0"):
            assert refused(case, "must be > 0"), case
        assert accepted("max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL") and accepted("max_leaves=SIZE_MAX")
        for case in ("max_leaves=2,d_levels=NULL", "max_leaves=2,d_siblings=NULL", "max_leaves=2,d_positions=NULL"):
            assert refused(case, "NULL buffer"), case
        assert accepted("counters=NULL")
        for case in ("n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "m=2^32", "m=SIZE_MAX", "k=SIZE_MAX/128/D+1", "k=SIZE_MAX"):
            assert refused(case, "size overflow"), case
        assert not refused("m=2^32-1", "size overflow")
        for buf in INS + OUTS[:6]:
            assert refused(buf + "=NULL", "NULL buffer"), buf
        for buf in OUTS[6:]:
            assert accepted(buf + "=NULL"), buf
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 13 and all(refused(c, "aligned") for c in misaligned)
        assert {"d_leaves+8", "d_offsets+4", "d_levels+8", "d_anchor_tree_ids+2", "d_anchor_counts+4", "d_anchor_ids+2", "d_leaf_ids+4", "d_anchor_roots+8",
                "d_leaves_out+8", "d_siblings+8", "d_n_bad_anchors+2", "d_n_bad+2", "d_n_hashed+4"} == set(misaligned)
        n = 0
        for o in OUTS:
            for i in INS + tuple(x for x in OUTS if x != o):
                case = "%s=%s+last" % (o, i)
                assert by[case][0] == -3 and "overlaps" in by[case][1] and o in by[case][1] and i in by[case][1], (o, i, by[case])
                assert accepted("%s=%s+end" % (o, i)), (o, i)
                n += 1
        assert n == 9 * 15
        assert refused("d_siblings=d_leaves-bytes+16", "d_siblings overlaps d_leaves") and accepted("d_siblings=d_leaves-bytes")
        assert accepted("k=0,d_leaves_out=d_leaves")


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_anchor.hip", os.path.join(CSRC, "_gen", "forest_anchor_test.s"))


def test_the_units_kernels_keep_the_projects_resource_conditions(compiled):
    """no private memory, no AGPRs, at least two waves per SIMD (tests/test_kernel_resources.py's conditions) for the unit's kernels — the
    anchor records, the gather of a level's children (once per arity), the roots, the opening records, the pieces (two index widths per
    arity); none of them hashes"""
    res, isa = compiled
    assert len([n for n in res if "k_fa_children" in n]) == 2 and len([n for n in res if "k_fa_openings" in n]) == 4
    for one in ("k_fa_anchor", "k_fa_roots", "k_fa_record"):
        assert len([n for n in res if one in n]) == 1, one
    assert len(res) == 9, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["occ"] >= 2 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_the_unit_hashes_through_the_librarys_digest_launch_and_the_forests_own_scratch():
    """every hashing kernel of the library has its row in the edge-value matrix (tests/edgecases.py); this unit adds none: the chains of
    partial nodes advance level by level through launch_merkle4, whose kernels the matrix names.  The scratch is the stream's pair,
    behind the forest's index; nothing is allocated and nothing waits."""
    from poseidon252_amd import build as b
    import edgecases
    assert "forest_anchor.hip" in b.SOURCES and "forest_anchor.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_anchor.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src) == ["k_fa_anchor", "k_fa_children", "k_fa_roots", "k_fa_record", "k_fa_openings"]
    for word in ("hades_permute", "node_digest_coop", "asm", "blockops.hpp", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy"):
        assert word not in code, word
    assert code.count("launch_merkle4(") == 1
    assert not re.search(r"\bk_(fo|fr|fc|path|merkle4)_\w+\s*[(<]", code)  # the neighbours' kernels through their launchers only
    assert set(edgecases.hashing_kernels()) <= set(edgecases.named_kernels())
    assert {"k_merkle4_coop", "k_merkle4_lat", "k_merkle4"} <= set(edgecases.named_kernels())
    api = open(os.path.join(CSRC, "api_forest.cpp")).read()
    body = api[api.index("static int forest_ragged_anchor_openings_device"):api.index("P252_MERKLE_PAIR(int, forest_ragged_anchor_openings_device_into")]
    assert body.count("with_forest_index(") == 1 and "with_stream_scratch(" not in body and "hipMalloc" not in body and "Synchronize" not in body
    assert "refuse_overlaps(" in body and "forest_shape_check(" in body


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    n_trees, max_leaves, m, k = 3, 100, 4, 5
    D = TS.depth(max_leaves, arity)
    method = ctx.merkle4_forest_ragged_anchor_openings_device if arity == 4 else ctx.merkle2_forest_ragged_anchor_openings_device
    args = dict(d_leaves=dev(n=120 * 4), d_offsets=dev(), d_levels=dev(n=(120 // (arity - 1) + n_trees * D) * 4), d_anchor_tree_ids=dev(i32), d_anchor_counts=dev(),
                d_anchor_ids=dev(i32), d_leaf_ids=dev(), d_anchor_roots=dev(n=m * 4), d_anchor_depths=dev(u8, n=m), d_leaves_out=dev(n=k * 4),
                d_siblings=dev(n=k * D * (arity - 1) * 4), d_positions=dev(u8, n=k * D), d_depths=dev(u8, n=k), d_n_bad_anchors=dev(i32), d_n_bad=dev(i32),
                d_n_hashed=dev())

    def call(a, m=m, k=k, max_leaves=max_leaves):
        return method(tag, a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_anchor_tree_ids"], a["d_anchor_counts"], m,
                      a["d_anchor_ids"], a["d_leaf_ids"], k, a["d_anchor_roots"], a["d_anchor_depths"], a["d_leaves_out"], a["d_siblings"],
                      a["d_positions"], a["d_depths"], a["d_n_bad_anchors"], a["d_n_bad"], a["d_n_hashed"])
    sym = "p252_merkle%d_forest_ragged_anchor_openings_device_into" % arity
    call(args)
    assert recorder.calls == [sym]  # the control: the library is reached, once, under this arity's symbol
    del recorder.calls[:]
    n_refused = 0
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call(bad)
        n_refused += 1
    assert n_refused == 16 and recorder.calls == []
    for name, short in (("d_offsets", dev(n=n_trees)), ("d_levels", dev(n=8)), ("d_anchor_tree_ids", dev(i32, n=m - 1)), ("d_anchor_counts", dev(n=m - 1)),
                        ("d_anchor_ids", dev(i32, n=k - 1)), ("d_leaf_ids", dev(n=k - 1)), ("d_anchor_roots", dev(n=m * 4 - 1)),
                        ("d_anchor_depths", dev(u8, n=m - 1)), ("d_leaves_out", dev(n=k * 4 - 1)), ("d_siblings", dev(n=k * D * (arity - 1) * 4 - 1)),
                        ("d_positions", dev(u8, n=k * D - 1)), ("d_depths", dev(u8, n=k - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call(dict(args, **{name: short}))
    for name, elem in (("d_offsets", 8), ("d_anchor_counts", 8), ("d_leaf_ids", 8), ("d_n_hashed", 8), ("d_anchor_depths", 1), ("d_positions", 1), ("d_depths", 1)):
        with pytest.raises(ValueError, match="%s needs %d-byte elements" % (name, elem)):
            call(dict(args, **{name: dev(i32)}))
    for name in ("d_anchor_tree_ids", "d_anchor_ids", "d_n_bad_anchors", "d_n_bad"):
        with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
            call(dict(args, **{name: dev()}))
    with pytest.raises(ValueError, match="d_siblings must be a torch tensor"):  # (only D == 0 or k == 0 has no rows)
        call(dict(args, d_siblings=None))
    with pytest.raises(ValueError, match="d_anchor_roots must be a torch tensor"):
        call(dict(args, d_anchor_roots=None))
    assert recorder.calls == []
    assert "arity" not in __import__("inspect").signature(method).parameters
    # the sizes the C call receives
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name == sym:
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    call(args)
    none = dict.fromkeys(("d_anchor_ids", "d_leaf_ids", "d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_n_bad_anchors", "d_n_bad", "d_n_hashed"))
    call(dict(args, **none), k=0)  # the roots alone
    call(dict(args, d_levels=None, d_siblings=None, d_positions=None), max_leaves=1)
    call(dict(args, d_anchor_tree_ids=None, d_anchor_counts=None, d_anchor_roots=None, d_anchor_depths=None), m=0)
    a, b, c, d = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    order = ("d_anchor_roots", "d_anchor_depths", "d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_n_bad_anchors", "d_n_bad", "d_n_hashed")
    assert a[2:] == (ptr(args["d_leaves"]), 120, ptr(args["d_offsets"]), n_trees, max_leaves, ptr(args["d_levels"]), ptr(args["d_anchor_tree_ids"]),
                     ptr(args["d_anchor_counts"]), m, ptr(args["d_anchor_ids"]), ptr(args["d_leaf_ids"]), k) + tuple(ptr(args[x]) for x in order) + (0,)
    assert b[10:] == (m, None, None, 0, ptr(args["d_anchor_roots"]), ptr(args["d_anchor_depths"])) + (None,) * 7 + (0,)
    assert c[6:8] == (1, None) and c[17:19] == (None, None) and c[19] == ptr(args["d_depths"])
    assert d[8:11] == (None, None, 0) and d[14:16] == (None, None) and d[16] == ptr(args["d_leaves_out"])


def test_the_helper_is_exported():
    import poseidon252_amd as P
    assert callable(P.forest_ragged_anchor_openings) and "forest_ragged_anchor_openings" in P.__all__


def test_the_model_imports_nothing_of_the_library():
    src = open(os.path.join(ROOT, "testsupport", "forestanchor.py")).read()
    imports = re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", src, re.M)
    assert set(imports) <= {"numpy", "."} and "poseidon252_amd" not in src and "torch" not in "".join(imports)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_anchor_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_anchor_bench")
