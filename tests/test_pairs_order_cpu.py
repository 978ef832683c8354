"""The order and the distinct (tree id, leaf id) pairs made on the device (p252_pairs_order_device_into, p252_pairs_unique_device_into;
csrc/pairs.hip) — what can be checked without a GPU: the numpy models the GPU tests compare the calls with (testsupport/pairsmodel.py:
the plain ones, and the device's method pass by pass) against each other and against forestsequential.stable_order; the symbols
declared, exported and mirrored; the host refusals as a table; the kernels' resources and the unit's text; the Python methods."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport import forestsequential as FS  # noqa: E402
from testsupport import pairsmodel as PM  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_pairs_order_device_into": 6, "p252_pairs_unique_device_into": 10}
KERNELS = {"k_po_load", "k_po_plan", "k_po_count", "k_po_scan", "k_po_scatter", "k_po_heads", "k_po_scan_heads", "k_po_compact"}


def _constants():
    src = open(os.path.join(CSRC, "pairs.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*constexpr unsigned\s+(PAIRS_\w+)\s*=\s*(\d+)u?\s*;", src, re.M)}


# ---- the models ----
def _random_pairs(rng, k, tree_bits, leaf_bits):
    t = rng.integers(0, 1 << tree_bits, size=k, dtype=np.uint64).astype(np.uint32)
    j = rng.integers(0, 1 << leaf_bits, size=k, dtype=np.uint64) if leaf_bits < 64 else rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)
    for i in range(1, k):  # half the pairs repeat an earlier one
        if rng.random() < 0.5:
            r = int(rng.integers(0, i))
            t[i], j[i] = t[r], j[r]
    return t, j


def test_the_models_agree_on_random_pairs_with_heavy_repeats():
    """the device-method model (tile counts, scans, ranked scatter, skipped passes; a small tile so that every input has several) gives
    the plain model's order and distinct pairs, and the plain order is forestsequential.stable_order's and valid"""
    rng = np.random.default_rng(0x9A125)
    for trial, (k, tb, lb) in enumerate([(1, 3, 3), (2, 1, 1), (97, 2, 3), (300, 16, 24), (1000, 3, 40), (513, 32, 64), (777, 0, 9)]):
        t, j = _random_pairs(rng, k, tb, lb)
        want = PM.order(t, j)
        assert np.array_equal(want, FS.stable_order(t, j)) and FS.order_is_valid(want, t, j)
        for tile in (64, 256):
            got, ran = PM.device_order(t, j, tile=tile)
            assert np.array_equal(got, want), (trial, tile)
            assert ran == PM.varying_passes(t, j) and len(ran) <= PM.PASSES
        wt, wj, wf = PM.unique(t, j)
        gt, gj, gf = PM.device_unique(t, j, tile=64)
        assert np.array_equal(gt, wt) and np.array_equal(gj, wj) and np.array_equal(gf, wf)
        # the distinct pairs are numpy's, and first is the lowest index of each
        packed = np.array([(int(a) << 64) | int(b) for a, b in zip(t, j)], dtype=object)
        distinct = sorted(set(packed.tolist()))
        assert [(int(a) << 64) | int(b) for a, b in zip(wt, wj)] == distinct
        assert wf.tolist() == [int(np.nonzero(packed == v)[0][0]) for v in distinct]
    # a None tree id is tree 0
    j = rng.integers(0, 50, size=200, dtype=np.uint64)
    assert np.array_equal(PM.order(None, j), PM.order(np.zeros(200, dtype=np.uint32), j))
    assert np.array_equal(PM.device_order(None, j, tile=64)[0], np.argsort(j, kind="stable"))


def test_both_parts_sort_as_unsigned_and_equal_keys_keep_their_order():
    j = np.array([2 ** 63, 5, 2 ** 64 - 1, 0, 2 ** 63], dtype=np.uint64)
    assert PM.order(None, j).tolist() == [3, 1, 0, 4, 2] and PM.device_order(None, j, tile=2)[0].tolist() == [3, 1, 0, 4, 2]
    t = np.array([0xFFFFFFFF, 0, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    j = np.array([0, 2 ** 64 - 1, 1, 0], dtype=np.uint64)
    assert PM.order(t, j).tolist() == [1, 2, 0, 3] == PM.device_order(t, j, tile=2)[0].tolist()
    same = PM.device_order(np.full(9, 7, dtype=np.uint32), np.full(9, 3, dtype=np.uint64), tile=4)
    assert same[0].tolist() == list(range(9)) and same[1] == [0]  # all keys equal: pass 0 alone, the identity
    u = PM.unique(np.full(9, 7, dtype=np.uint32), np.full(9, 3, dtype=np.uint64))
    assert [x.tolist() for x in u] == [[7], [3], [0]]


def test_a_pass_runs_iff_its_byte_varies():
    for b in range(PM.PASSES):
        j = np.zeros(10, dtype=np.uint64)
        t = np.zeros(10, dtype=np.uint32)
        vals = np.array([3, 1, 2, 1, 0, 255, 3, 3, 128, 127], dtype=np.uint64)
        if b < 8:
            j = (vals << np.uint64(8 * b)) | np.uint64(0x0101010101010101 & ~(0xFF << (8 * b)))
        else:
            t = (vals << np.uint64(8 * (b - 8))).astype(np.uint32)
        assert PM.varying_passes(t, j) == [b]
        assert np.array_equal(PM.device_order(t, j, tile=4)[0], np.argsort(vals, kind="stable"))


def test_the_model_imports_nothing_of_the_library():
    src = open(os.path.join(ROOT, "testsupport", "pairsmodel.py")).read()
    imports = re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", src, re.M)
    assert set(imports) == {"numpy"} and "poseidon252_amd" not in src and "torch" not in src


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    from poseidon252_amd import _lib
    import poseidon252_amd as P
    raw, header = check_abi_symbols(SYMBOLS)
    listed = raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    assert "p252_pairs_order_device_into" in listed and "p252_pairs_unique_device_into" in listed
    doc = raw[raw.index("/* ---- the order of (tree id, leaf id) pairs"):raw.index("int p252_pairs_order_device_into")]
    for word in ("p252_trim", "UNSIGNED", "d_first", "NULL", "bytes a pair", "k alone", "captured graph", "2^32", "left alone"):
        assert word in doc, word
    # the order of _lib.PROTOTYPES is the header's
    order = [n for n in re.findall(r"\b(p252_\w+)\s*\(", header) if n in _lib.PROTOTYPES]
    assert list(dict.fromkeys(order)) == list(_lib.PROTOTYPES)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration
    hpp = open(os.path.join(ROOT, "include", "poseidon252.hpp")).read()
    assert "p252_pairs_order_device_into(" in hpp and "p252_pairs_unique_device_into(" in hpp
    assert "inline void pairs_order_device(" in hpp and "inline void pairs_unique_device(" in hpp
    for name in ("pairs_order", "pairs_unique"):
        assert callable(getattr(P, name)) and name in P.__all__
    from poseidon252_amd import hash as H
    assert len(H._PER_ARITY_STEMS) == 17  # neither call depends on an arity


def test_the_scratch_figure_of_the_header_is_the_codes():
    c = _constants()
    assert c["PAIRS_TILE"] == c["PAIRS_BLOCK"] * c["PAIRS_ROUNDS"] and c["PAIRS_DIGITS"] == 256 and c["PAIRS_PASSES"] == PM.PASSES
    raw = open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read()
    per_pair = 32 + c["PAIRS_DIGITS"] * 4 / c["PAIRS_TILE"]
    assert "%g bytes a pair" % per_pair in raw and "256 words per {:,} pairs".format(c["PAIRS_TILE"]) in raw
    h = open(os.path.join(CSRC, "pairs.h")).read()
    assert "%g bytes a pair" % per_pair in h and "k * 16" in h and "n_tiles * PAIRS_DIGITS * 4" in h


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("pairs_refusal_table", tmp_path_factory.mktemp("pairs_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "pairs_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for sym, buffers, optional in (("p252_pairs_order_device_into", 3, {"d_tree_ids=NULL"}),
                                   ("p252_pairs_unique_device_into", 7, {"d_tree_ids=NULL", "d_tree_ids_out=NULL", "d_leaf_ids_out=NULL",
                                                                         "d_indices_out=NULL", "d_first=NULL"})):
        by = {r[1]: r[2:] for r in table if r[0] == sym}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and refused("k=0", "must be > 0") and accepted("k=1")
        for case in ("k=2^32", "k=SIZE_MAX/16+1", "k=SIZE_MAX"):
            assert refused(case, "below 2^32"), case
        assert by["k=2^32-1"][0] == -3 and "below 2^32" not in by["k=2^32-1"][1]  # (the addresses of the table overlap at that size)
        nulls = [c for c in by if re.fullmatch(r"d_\w+=NULL", c)]
        assert len(nulls) == buffers
        for c in nulls:
            assert accepted(c) if c in optional else refused(c, "NULL buffer"), c
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == buffers and all(refused(c, "aligned") for c in misaligned)
        overlaps = [c for c in by if re.fullmatch(r"d_\w+=d_\w+(\+[\d*]+)?", c)]
        assert len(overlaps) == (4 if buffers == 3 else 10)
        for c in overlaps:
            out, other = re.fullmatch(r"(d_\w+)=(d_\w+?)(\+[\d*]+)?", c).groups()[:2]
            assert accepted(c) if c.endswith(("8*9", "4*10")) else refused(c, "%s overlaps %s" % (out, other)), c
    order = {r[1]: r[2:] for r in table if r[0] == "p252_pairs_order_device_into"}
    assert order["d_tree_ids=NULL,d_order=d_leaf_ids"][0] == -3 and "d_order overlaps d_leaf_ids" in order["d_tree_ids=NULL,d_order=d_leaf_ids"][1]
    unique = {r[1]: r[2:] for r in table if r[0] == "p252_pairs_unique_device_into"}
    assert unique["one output: d_first"] == unique["control"] == unique["one output: d_indices_out"]
    assert unique["no array output"][0] == -3 and "at least one of" in unique["no array output"][1]


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("pairs.hip", os.path.join(CSRC, "_gen", "pairs_test.s"))


def test_the_units_kernels_have_no_private_memory_and_keep_eight_waves(compiled):
    """no private memory, no AGPRs and at least 8 waves per SIMD for every k_po_* kernel; records move as one dwordx4 per lane"""
    res, isa = compiled
    assert {re.search(r"k_po_[a-z_]+?(?=E[A-Zv])", name).group(0) for name in res} == KERNELS and len(res) == len(KERNELS), sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["occ"] >= 8, (name, v)
    assert "scratch_" not in isa
    scatter = isa[isa.index("k_po_scatter"):]
    scatter = scatter[:scatter.index("s_endpgm")]
    assert "global_load_dwordx4" in scatter and "global_store_dwordx4" in scatter
    assert "ds_add" not in scatter and "atomic" not in scatter  # the ranks are computed, not claimed


def test_the_unit_sorts_by_itself_and_never_waits():
    """The text of pairs.hip.  None of the words of an allocation, a host wait, a copy, inline assembly, another library's sort or
    the permutation; no blockops.hpp.  How "no loop whose exit depends on global memory another block writes" was checked: the file
    was read — it has no `while`, no `do` and no `for (;;)` at all (asserted below), and every `for` loop it has is counted: each has
    a bound that is a compile-time constant or a kernel argument (n_tiles), none reads memory in its condition (asserted: the
    condition of every `for` holds no `[`, no `*` dereference and no `->`).  The scatter's rank uses no LDS atomic: the one atomicAdd
    of the unit is k_po_count's, the one atomicOr is k_po_load's."""
    from poseidon252_amd import build as b
    assert "pairs.hip" in b.SOURCES and "pairs.h" in b.HEADERS
    src = open(os.path.join(CSRC, "pairs.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert set(re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src)) == KERNELS
    for word in ("hipMalloc", "Synchronize", "hipMemcpy", "asm", "rocprim", "hipcub", "thrust", "cub::", "hades_permute", "node_digest",
                 "blockops.hpp", "atomicCAS", "cooperative", "grid.sync", "volatile", "__threadfence"):
        assert word not in src, word
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', code) == ["hip/hip_runtime.h", "pairs.h"]
    assert not re.search(r"\b(while|do|goto)\b", code) and not re.search(r"for\s*\(\s*;\s*;", code)
    loops = re.findall(r"\bfor\s*\(([^;]*);([^;]*);", code)
    assert len(loops) >= 10
    for _, cond in loops:
        assert not re.search(r"\[|->|\*\s*\w", cond), cond
    body = lambda name: code[code.index(name + "("):].split("\n}\n")[0]  # noqa: E731
    assert code.count("atomicAdd(") == 1 and "atomicAdd(" in body("k_po_count") and code.count("atomicOr(") == 3 and "atomicOr(" in body("k_po_load")
    scatter = body("k_po_scatter")
    assert scatter.count("__ballot(") == 2 and "__popcll(" in scatter and "lanes_below()" in scatter and "atomic" not in scatter
    # a skipped pass: its three kernels leave at once on the plan's word
    for name in ("k_po_count", "k_po_scan", "k_po_scatter"):
        assert re.search(r"\{\s*if \(!ctl\[PO_ACTIVE \+ pass\]\) return;", body(name)), name
    api = open(os.path.join(CSRC, "api_forest.cpp")).read()
    for sym in SYMBOLS:
        entry = api[api.index("int %s(" % sym):]
        entry = entry[:entry.index("\n}\n")]
        assert entry.count("with_stream_scratch(") == 1 and "refuse_overlaps(" in entry and "hipMalloc" not in entry and "Synchronize" not in entry


# ---- the Python methods ----
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch):
    ctx = _no_device_context()
    i32 = torch.int32
    k = 9
    o_args = dict(d_tree_ids=dev(i32), d_leaf_ids=dev(), d_order=dev(i32))
    u_args = dict(d_tree_ids=dev(i32), d_leaf_ids=dev(), d_n_unique=dev(), d_tree_ids_out=dev(i32), d_leaf_ids_out=dev(), d_indices_out=dev(i32),
                  d_first=dev(i32))

    def order(a):
        return ctx.pairs_order_device(a["d_tree_ids"], a["d_leaf_ids"], k, a["d_order"])

    def unique(a):
        return ctx.pairs_unique_device(a["d_tree_ids"], a["d_leaf_ids"], k, a["d_n_unique"], d_tree_ids_out=a["d_tree_ids_out"],
                                       d_leaf_ids_out=a["d_leaf_ids_out"], d_indices_out=a["d_indices_out"], d_first=a["d_first"])
    order(o_args), unique(u_args), order(dict(o_args, d_tree_ids=None)), unique(dict(u_args, d_tree_ids=None, d_first=None))
    assert recorder.calls == ["p252_pairs_order_device_into", "p252_pairs_unique_device_into"] * 2  # the control: the library is reached
    del recorder.calls[:]
    for call, args, wide, narrow in ((order, o_args, ("d_leaf_ids",), ("d_tree_ids", "d_order")),
                                     (unique, u_args, ("d_leaf_ids", "d_leaf_ids_out", "d_n_unique"),
                                      ("d_tree_ids", "d_tree_ids_out", "d_indices_out", "d_first"))):
        for where, bad in with_cpu_tensor(args):
            with pytest.raises(ValueError, match=where + " is on cpu"):
                call(dict(args, **bad))
        for name in wide:
            if name != "d_n_unique":
                with pytest.raises(ValueError, match=name + " holds"):
                    call(dict(args, **{name: dev(n=k - 1)}))
            with pytest.raises(ValueError, match=name + " needs 8-byte elements"):
                call(dict(args, **{name: dev(i32, n=64)}))
        for name in narrow:
            with pytest.raises(ValueError, match=name + " holds"):
                call(dict(args, **{name: dev(i32, n=k - 1)}))
            with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
                call(dict(args, **{name: dev(n=64)}))
    with pytest.raises(ValueError, match="d_order must be a torch tensor"):
        order(dict(o_args, d_order=None))
    with pytest.raises(ValueError, match="d_leaf_ids must be a torch tensor"):
        unique(dict(u_args, d_leaf_ids=None))
    with pytest.raises(ValueError, match="d_n_unique must be a torch tensor"):
        unique(dict(u_args, d_n_unique=None))
    assert recorder.calls == []
    # the sizes the C calls receive
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name in SYMBOLS:
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    other = type("S", (), {"cuda_stream": 77})()
    order(o_args)
    ctx.pairs_order_device(None, o_args["d_leaf_ids"], k, o_args["d_order"], stream=other)
    unique(u_args)
    ctx.pairs_unique_device(None, u_args["d_leaf_ids"], k, u_args["d_n_unique"], d_indices_out=u_args["d_indices_out"], stream=other)
    a, b, c, d = seen
    po, pu = (lambda n: o_args[n].data_ptr()), (lambda n: u_args[n].data_ptr())
    assert a[1:] == (po("d_tree_ids"), po("d_leaf_ids"), k, po("d_order"), 0)
    assert b[1:] == (None, po("d_leaf_ids"), k, po("d_order"), 77)
    assert c[1:] == (pu("d_tree_ids"), pu("d_leaf_ids"), k, pu("d_tree_ids_out"), pu("d_leaf_ids_out"), pu("d_indices_out"), pu("d_first"),
                     pu("d_n_unique"), 0)
    assert d[1:] == (None, pu("d_leaf_ids"), k, None, None, pu("d_indices_out"), None, pu("d_n_unique"), 77)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_pairs_order_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("pairs_order_bench")
