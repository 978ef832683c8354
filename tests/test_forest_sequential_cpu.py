"""Leaf updates of a ragged forest applied in order, each with its witness (p252_merkle{4,2}_forest_ragged_update_sequential_device_into;
csrc/forest_sequential.hip) — what can be checked without a GPU: the two numpy models the GPU tests compare the call with
(testsupport/forestsequential.py: one by one, and level-parallel as the device works) against each other and against the oracle's
trees; the digest count; the symbols declared, exported and mirrored; the host refusals as a table; the kernels' resources; the Python
methods."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
import edgecases as E  # noqa: E402
from testsupport import forestsequential as FS  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_ragged_update_sequential_device_into": 23, "p252_merkle2_forest_ragged_update_sequential_device_into": 23}
KERNELS = {"k_sq_check", "k_sq_gather", "k_sq_rank", "k_sq_finish"}


def _tag(arity):
    from poseidon252_amd import merkle
    return merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()


# ---- the two models ----
@pytest.mark.parametrize("arity", [4, 2])
def test_the_two_models_agree_on_random_forests_with_repeated_pairs(oracle_mod, arity):
    """random ragged forests (an empty tree among them), updates that repeat pairs heavily and a few bad ones: the level-parallel model
    returns what one-by-one application returns, both leave the same forest, that forest is the oracle's tree of the final leaves, and
    every witness re-hashes to the roots before and after"""
    tag = _tag(arity)
    digest = lambda kids: oracle_mod.hash_batch(tag, kids, arity, 1)  # noqa: E731
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    rng = np.random.default_rng(1000 + arity)
    n_digests = [0]

    def counted(kids):
        n_digests[0] += len(kids)
        return digest(kids)
    for trial in range(6):
        sizes = [int(x) for x in rng.choice([0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33], size=int(rng.integers(1, 7)))]
        if not any(sizes):
            sizes[0] = 5
        top = max(sizes)
        leaves = oracle_mod.fill_random(77 * trial + arity, sum(sizes))
        k = int(rng.integers(1, 60))
        tid = rng.integers(0, len(sizes) + (trial % 2), size=k)  # (odd trials: an unknown tree id among them)
        lid = np.array([int(rng.integers(0, max(sizes[t] if t < len(sizes) else 1, 1) + (trial % 3 == 0))) for t in tid])
        repeat = rng.random(k) < 0.5  # half the updates repeat an earlier pair
        for i in range(1, k):
            if repeat[i]:
                j = int(rng.integers(0, i))
                tid[i], lid[i] = tid[j], lid[j]
        new = oracle_mod.fill_random(9000 + trial, k)
        order = FS.stable_order(tid, lid)
        assert FS.order_is_valid(order, tid, lid)
        one, two = FS.build_forest(leaves, sizes, arity, digest), FS.build_forest(leaves, sizes, arity, digest)
        n_digests[0] = 0
        A = FS.sequential_model(one, tid, lid, new, top, arity, counted, E.reduce_mod_p)
        assert n_digests[0] == A.n_hashed == sum(int(TS.depth(sizes[t], arity)) for t, g in zip(tid, FS.good_updates(sizes, tid, lid)) if g)
        B = FS.level_parallel_model(two, tid, lid, new, order, top, arity, digest, E.reduce_mod_p)
        assert A.same(B), (arity, trial)
        assert A.n_bad == int((~FS.good_updates(sizes, tid, lid)).sum())
        for x, y in zip(FS.forest_arrays(one, E.reduce_mod_p), FS.forest_arrays(two, E.reduce_mod_p)):
            assert np.array_equal(x, y)
        # the forest afterwards is the oracle's tree of the final leaves
        for t, n in enumerate(sizes):
            if n > 1:
                root, levels = tree(tag, one[t][0], want_levels=True)[:2]
                assert np.array_equal(root, one[t][-1][0]) and np.array_equal(np.asarray(levels).reshape(-1, 4), np.concatenate(one[t][1:]))
        # every witness re-hashes to the two roots; the chain of roots of a tree is unbroken
        last = {}
        for i in range(k):
            if A.dep[i] == FS.BAD_DEPTH:
                assert not (A.old[i].any() or A.sib[i].any() or A.before[i].any() or A.after[i].any())
                continue
            for leaf, want in ((A.old[i], A.before[i]), (new[i], A.after[i])):
                node = leaf
                for l in range(int(A.dep[i])):
                    kids = np.insert(A.sib[i, l], int(A.pos[i, l]), node, axis=0)
                    node = np.asarray(digest(kids.reshape(1, arity, 4))).reshape(4)
                if A.dep[i] == 0:
                    node = E.reduce_mod_p(node.reshape(1, 4))[0]
                assert np.array_equal(node, want), (arity, trial, i)
            assert not A.sib[i, int(A.dep[i]):].any() and not A.pos[i, int(A.dep[i]):].any()
            if int(tid[i]) in last:
                assert np.array_equal(A.before[i], A.after[last[int(tid[i])]])
            last[int(tid[i])] = i


def test_the_order_rule():
    tid, lid = np.array([1, 0, 1, 0, 1]), np.array([3, 2, 3, 2, 0])
    order = FS.stable_order(tid, lid)
    assert order.tolist() == [1, 3, 4, 0, 2] and FS.order_is_valid(order, tid, lid)
    for bad in ([1, 3, 4, 0, 0], [1, 3, 4, 0, 5], [4, 0, 2, 1, 3], [1, 3, 0, 2, 4], [3, 1, 4, 0, 2], [1, 3, 4, 0]):
        assert not FS.order_is_valid(bad, tid, lid), bad
    # 64-bit leaf ids sort as unsigned
    assert FS.stable_order([0, 0], np.array([2 ** 63, 5], dtype=np.uint64)).tolist() == [1, 0]


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    from poseidon252_amd import _lib
    raw, header = check_abi_symbols(SYMBOLS)
    listed = raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    assert "_forest_ragged_update_sequential_device_into" in listed
    doc = raw[raw.index("/* ---- sequential updates:"):raw.index("int p252_merkle4_forest_ragged_update_sequential_device_into")]
    for word in ("p252_trim", "0xFF", "d_order", "byte for byte", "mod p", "bytes an update", "permutation", "*d_n_bad += k"):
        assert word in doc, word
    # the order of _lib.PROTOTYPES is the header's
    order = [n for n in re.findall(r"\b(p252_\w+)\s*\(", header) if n in _lib.PROTOTYPES]
    assert list(dict.fromkeys(order)) == list(_lib.PROTOTYPES)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration
    hpp = open(os.path.join(ROOT, "include", "poseidon252.hpp")).read()
    assert "X(N, forest_ragged_update_sequential_device_into)" in hpp and "inline void merkle_forest_ragged_update_sequential_device(" in hpp


def test_the_helper_is_exported_and_no_arity_method_is_added():
    import poseidon252_amd as P
    from poseidon252_amd import Context, hash as H
    name = "forest_ragged_update_sequential"
    assert callable(getattr(P, name)) and name in P.__all__ and inspect.signature(getattr(P, name)).parameters["arity"].default == 4
    stem = "forest_ragged_update_sequential_device"
    assert not hasattr(Context, "merkle_" + stem) and stem not in H._PER_ARITY_STEMS and len(H._PER_ARITY_STEMS) == 17
    for arity in (4, 2):
        m = getattr(Context, "merkle%d_%s" % (arity, stem))
        assert inspect.isfunction(m) and m.__name__ == "merkle%d_%s" % (arity, stem) and "arity" not in inspect.signature(m).parameters
        assert "p252_merkle%d_" % arity in m.__doc__


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("sequential_refusal_table", tmp_path_factory.mktemp("sequential_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "sequential_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_ragged_update_sequential_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and refused("tag=NULL", "NULL buffer")
        for case in ("k=0", "n_leaves=0", "n_trees=0", "max_leaves=0"):
            assert refused(case, "must be > 0"), case
        for case in ("k=2^32", "k=SIZE_MAX", "max_leaves=2^32", "max_leaves=SIZE_MAX"):
            assert refused(case, "below 2^32"), case
        assert accepted("max_leaves=2^32-1") and by["k=2^32-1"][0] == -3 and "below 2^32" not in by["k=2^32-1"][1]
        assert accepted("optional=NULL") and accepted("max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL")
        for case in ("max_leaves=2,d_levels=NULL", "max_leaves=2,d_siblings=NULL", "max_leaves=2,d_positions=NULL"):
            assert refused(case, "NULL buffer"), case
        for case in ("n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2"):
            assert refused(case, "size overflow"), case
        overlaps = [c for c in by if re.fullmatch(r"d_\w+=d_\w+(\+[\d*]+)?", c)]
        assert len(overlaps) == 11
        for c in overlaps:
            out, other = re.fullmatch(r"(d_\w+)=(d_\w+?)(\+[\d*]+)?", c).groups()[:2]
            assert accepted(c) if c.endswith("32*9") else refused(c, "%s overlaps %s" % (out, other)), c
        nulls = [c for c in by if re.fullmatch(r"d_\w+=NULL", c)]
        optional = {"d_old_leaves=NULL", "d_roots_before=NULL", "d_roots=NULL", "d_n_bad=NULL", "d_n_hashed=NULL"}
        assert len(nulls) == 16
        for c in nulls:
            assert accepted(c) if c in optional else refused(c, "NULL buffer"), c
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 14 and all(refused(c, "aligned") for c in misaligned)


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_sequential.hip", os.path.join(CSRC, "_gen", "forest_sequential_test.s"))


def test_the_units_kernels_have_no_private_memory_and_keep_eight_waves(compiled):
    """no private memory, no AGPRs and at least 8 waves per SIMD for every kernel of the unit: the check, the gather and the merge rank
    (the last two once per arity) and the finish"""
    res, isa = compiled
    for one, n in (("k_sq_check", 1), ("k_sq_gather", 2), ("k_sq_rank", 2), ("k_sq_finish", 1)):
        assert len([name for name in res if one in name]) == n, one
    assert len(res) == 6, sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64 and v["occ"] >= 8, (name, v)
    assert "scratch_" not in isa
    gather = isa[isa.index("k_sq_gather"):]
    assert "global_load_dwordx4" in gather and "global_store_dwordx4" in gather  # scalars as two 16-byte accesses


def test_the_unit_hashes_through_one_digest_launch_and_the_streams_scratch():
    """every hashing kernel of the library has its row in the edge-value matrix (tests/edgecases.py); this unit adds none: the digests go
    through launch_merkle4, at exactly one call site.  The forest's index is the ragged forest's own launcher; the scratch is the
    stream's pair; nothing is allocated, nothing waits and nothing is sorted."""
    from poseidon252_amd import build as b
    assert "forest_sequential.hip" in b.SOURCES and "forest_sequential.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_sequential.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    mine = set(re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src))
    assert mine == KERNELS
    assert not (E.hashing_kernels() & mine) and set(E.hashing_kernels()) <= set(E.named_kernels())
    for word in ("hades_permute", "node_digest_coop", "asm", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "atomicCAS",
                 "sort", "cub::", "thrust"):
        assert word not in code, word
    assert code.count("launch_merkle4(") == 1
    assert not re.search(r"\bk_(fm|mp|fr|fo|fu|fa|rg)_\w+\s*[(<]", code)  # the neighbours' kernels through their launchers only
    # every kernel but the check leaves at once after an invalid order
    for name in KERNELS - {"k_sq_check"}:
        body = code[code.index(name + "("):]
        body = body[:body.index("\n}\n")]
        assert "ctr[SQ_BAD]" in body, name
    api = open(os.path.join(CSRC, "api_forest.cpp")).read()
    body = api[api.index("static int forest_ragged_update_sequential_device"):api.index("P252_MERKLE_PAIR(int, forest_ragged_update_sequential_device_into")]
    assert body.count("with_forest_index(") == 1 and "with_stream_scratch(" not in body and "forest_shape_check(" in body
    assert "refuse_overlaps(" in body and "hipMalloc" not in body and "Synchronize" not in body


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    n_trees, max_leaves, k = 3, 100, 9
    D = TS.depth(max_leaves, arity)
    update = getattr(ctx, "merkle%d_forest_ragged_update_sequential_device" % arity)
    args = dict(d_leaves=dev(n=120 * 4), d_offsets=dev(), d_levels=dev(n=(120 // (arity - 1) + n_trees * D) * 4), d_tree_ids=dev(i32), d_leaf_ids=dev(),
                d_new_leaves=dev(n=k * 4), d_order=dev(i32), d_siblings=dev(n=k * D * (arity - 1) * 4), d_positions=dev(u8, n=k * D), d_depths=dev(u8, n=k),
                d_roots_after=dev(n=k * 4), d_old_leaves=dev(n=k * 4), d_roots_before=dev(n=k * 4), d_roots=dev(n=n_trees * 4), d_n_bad=dev(i32),
                d_n_hashed=dev())

    def call(a, max_leaves=max_leaves):
        return update(tag, a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_tree_ids"], a["d_leaf_ids"], a["d_new_leaves"],
                      a["d_order"], k, a["d_siblings"], a["d_positions"], a["d_depths"], a["d_roots_after"], d_old_leaves=a["d_old_leaves"],
                      d_roots_before=a["d_roots_before"], d_roots=a["d_roots"], d_n_bad=a["d_n_bad"], d_n_hashed=a["d_n_hashed"])
    sym = "p252_merkle%d_forest_ragged_update_sequential_device_into" % arity
    call(args)
    assert recorder.calls == [sym]  # the control: the library is reached, once, under this arity's symbol
    del recorder.calls[:]
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call(dict(args, **bad))
    for name, short in (("d_offsets", dev(n=n_trees)), ("d_tree_ids", dev(i32, n=k - 1)), ("d_leaf_ids", dev(n=k - 1)), ("d_new_leaves", dev(n=k * 4 - 1)),
                        ("d_order", dev(i32, n=k - 1)), ("d_siblings", dev(n=k * D * (arity - 1) * 4 - 1)), ("d_positions", dev(u8, n=k * D - 1)),
                        ("d_depths", dev(u8, n=k - 1)), ("d_roots_after", dev(n=k * 4 - 1)), ("d_old_leaves", dev(n=k * 4 - 1)),
                        ("d_roots_before", dev(n=k * 4 - 1)), ("d_roots", dev(n=n_trees * 4 - 1)), ("d_levels", dev(n=8))):
        with pytest.raises(ValueError, match=name + " holds"):
            call(dict(args, **{name: short}))
    for name in ("d_leaf_ids", "d_n_hashed"):
        with pytest.raises(ValueError, match=name + " needs 8-byte elements"):
            call(dict(args, **{name: dev(i32, n=64)}))
    for name in ("d_tree_ids", "d_order", "d_n_bad"):
        with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
            call(dict(args, **{name: dev(n=64)}))
    with pytest.raises(ValueError, match="d_siblings must be a torch tensor"):
        call(dict(args, d_siblings=None))
    assert recorder.calls == []
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
    call(dict(args, d_levels=None, d_siblings=None, d_positions=None, d_old_leaves=None, d_roots_before=None, d_roots=None, d_n_bad=None,
              d_n_hashed=None), max_leaves=1)
    a, b = seen
    ptr = lambda name: args[name].data_ptr()  # noqa: E731
    assert a[2:] == (ptr("d_leaves"), 120, ptr("d_offsets"), n_trees, max_leaves, ptr("d_levels"), ptr("d_tree_ids"), ptr("d_leaf_ids"),
                     ptr("d_new_leaves"), ptr("d_order"), k, ptr("d_old_leaves"), ptr("d_siblings"), ptr("d_positions"), ptr("d_depths"),
                     ptr("d_roots_before"), ptr("d_roots_after"), ptr("d_roots"), ptr("d_n_bad"), ptr("d_n_hashed"), 0)
    assert b[6:8] == (1, None) and b[13:16] == (None, None, None) and b[17] is None and b[19:22] == (None, None, None)


def test_the_convenience_refuses_a_wrong_arity_before_anything_else():
    from poseidon252_amd import merkle
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        merkle.forest_ragged_update_sequential(None, None, None, 1, 1, None, [0], [0], np.zeros((1, 4), dtype=np.uint64), arity=3)


def test_the_model_imports_nothing_of_the_library():
    src = open(os.path.join(ROOT, "testsupport", "forestsequential.py")).read()
    imports = re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", src, re.M)
    assert set(imports) <= {"numpy", "bisect", "."} and "poseidon252_amd" not in src and "torch" not in "".join(imports)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_sequential_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_sequential_bench")
