"""The openings of marked leaves kept current across appends to a forest kept only as its frontiers
(p252_merkle{4,2}_forest_frontier_append_witness_device_into; csrc/forest_witness.hip) — what can be checked without a GPU: the numpy
model the GPU tests compare the call with (testsupport/forestwitness.py) against openings cut out of full builds by the oracle, for
every small tree, append and leaf; the symbols declared, exported and mirrored; the host refusals as a table; the C++ mirror; the unit
hashes nothing and its one kernel uses no private memory; the Python methods validate every buffer before the library is reached."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport import forestfrontier as FF  # noqa: E402
from testsupport import forestwitness as FW  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_frontier_append_witness_device_into": 21, "p252_merkle2_forest_frontier_append_witness_device_into": 21}
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


def _openings(builds, arity, n):
    """the openings of all n leaves of the build of n, at the stride of MAX_LEAVES"""
    leaves, built = builds[arity]
    D = TS.depth(MAX_LEAVES, arity)
    return [FW.opening_of(leaves, built[n][1], n, p, arity, D) for p in range(n)] if n else []


@pytest.mark.parametrize("arity", [4, 2])
def test_model_refresh_equals_the_opening_out_of_the_larger_build(oracle_mod, builds, arity):
    """every n in 0 .. 70, every m in 0 .. 20 and EVERY p < n + m: the carried ones start from the opening at n, the new ones from
    garbage; n = 0, 1, A^d - 1, A^d, A^d + 1 and appends that add one and two levels are all among them"""
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES, arity)
    cut = {n: _openings(builds, arity, n) for n in range(N_MAX + M_MAX + 1)}
    garbage = FW.Witness(arity, D, np.full(4, 7, np.uint64), np.full((D, arity - 1, 4), 9, np.uint64), np.full(D, 3, np.uint8), 5)
    grew = set()
    for n in range(N_MAX + 1):
        old = _state(builds, arity, n)
        for m in range(M_MAX + 1):
            computed = FW.computed_levels(old, leaves[n:n + m], digest) if m else None
            for p in range(n + m):
                got = FW.refresh(cut[n][p] if p < n else garbage, p, old, leaves[n:n + m], digest, computed=computed)
                assert got == cut[n + m][p], (arity, n, m, p)
            grew.add(TS.depth(n + m, arity) - TS.depth(n, arity))
    assert {0, 1, 2} <= grew
    # an opening cut out of a build re-hashes to that build's root, and its rows from the depth on are zero
    for n in (1, 2, arity ** 2, arity ** 2 + 1, 70):
        for p in (0, n // 2, n - 1):
            w = cut[n][p]
            cur = leaves[p]
            for l in range(w.depth):
                kids = np.insert(w.siblings[l], int(w.positions[l]), cur, axis=0)
                cur = np.asarray(digest(kids.reshape(1, arity, 4))).reshape(4)
            want = FF.reduce_leaf(leaves[0]) if n == 1 else built[n][0]
            assert np.array_equal(FF.reduce_leaf(cur) if n == 1 else cur, want) and not w.siblings[w.depth:].any() and not w.positions[w.depth:].any(), (arity, n, p)


@pytest.mark.parametrize("arity", [4, 2])
def test_model_bad_and_stale_rules(oracle_mod, builds, arity):
    leaves, _ = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES, arity)
    n, m = 17, 5
    old, good = _state(builds, arity, n), _openings(builds, arity, n)
    bad = FW.Witness(arity, D)
    assert bad.bad() and bad.depth == 0xFF and not bad.leaf.any() and not bad.siblings.any() and not bad.positions.any()
    # not in the tree: at n', past it, and the same where nothing is appended
    for p in (n + m, n + m + 1, 10 ** 12):
        assert FW.refresh(good[3], p, old, leaves[n:n + m], digest) == bad
    assert FW.refresh(good[3], n, old, leaves[:0], digest) == bad
    # a carried witness with a depth byte that is not depth(n): bad when the tree grows, left as it is when it does not
    for depth in (TS.depth(n, arity) - 1, TS.depth(n, arity) + 1, 0, 0xFF):
        stale = good[3].copy()
        stale.depth = depth
        assert FW.refresh(stale, 3, old, leaves[n:n + m], digest) == bad
        assert FW.refresh(stale, 3, old, leaves[:0], digest) == stale
    # a leaf the call brings: whatever the input holds
    want = _openings(builds, arity, n + m)
    for seed in (bad, good[3]):
        assert FW.refresh(seed, n + 1, old, leaves[n:n + m], digest) == want[n + 1]
    # the argument is never changed
    before = good[3].copy()
    FW.refresh(good[3], 3, old, leaves[n:n + m], digest)
    assert good[3] == before


def test_model_byte_count_equals_a_witness_by_witness_count():
    """pass_bytes (what the bench tool divides by its times) against the rule walked one witness and one row at a time"""
    rng = np.random.default_rng(5)
    for arity in (4, 2):
        D = TS.depth(MAX_LEAVES, arity)
        sizes, adds = rng.integers(0, 60, 30), rng.integers(0, 25, 30) * (rng.random(30) < 0.7)
        tid = rng.integers(0, 30, 400)
        lid = (rng.random(400) * np.maximum(sizes + adds, 1)[tid]).astype(np.int64)
        read, written = 400 * D * 29, 0
        for t, p in zip(tid, lid):
            n, nn = int(sizes[t]), int(sizes[t] + adds[t])
            if nn == n:
                continue
            written += 1  # the depth byte
            if p >= n:
                read, written = read + 32, written + 32  # the leaf
            for l in range(D):
                node, f, c = p // arity ** l, n // arity ** l, -(-nn // arity ** l)
                if l >= TS.depth(nn, arity):
                    written += ((arity - 1) * 32 + 1) * (p >= n)
                    continue
                if p < n and node // arity < n // arity ** (l + 1):
                    continue
                written += 1
                for x in range(node - node % arity, node - node % arity + arity):
                    if x != node and not (x < f and p < n):
                        read, written = read + 32 * (x < c), written + 32
        assert FW.pass_bytes(arity, D, sizes, adds, tid, lid) == (read, written), arity


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    raw, header = check_abi_symbols(SYMBOLS)
    assert "forest_frontier_append_witness_device_into" in raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    assert not any("frontier" in s for s in re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("witness_refusal_table", tmp_path_factory.mktemp("witness_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "witness_refusals")


STATE = ("d_counts", "d_frontier", "d_roots", "d_n_bad", "d_n_hashed")
INPUTS = ("d_add", "d_add_offsets")
IDS = ("d_wit_tree_ids", "d_wit_leaf_ids")
MINE = ("d_wit_leaves", "d_wit_siblings", "d_wit_positions", "d_wit_depths", "d_n_bad_witness")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_frontier_append_witness_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        # everything the plain call refuses
        assert by["ctx=NULL"][0] == -3 and by["n_trees=0,k=0"] == (0, "") and by["n_trees=0,k=0,max_leaves=0"] == (0, "")
        assert accepted("n_trees=0") and accepted("n_trees=0,state=NULL") and refused("n_trees=0,max_leaves=0", "max_leaves")
        assert refused("max_leaves=0", "max_leaves") and accepted("max_leaves=1") and accepted("max_leaves=SIZE_MAX")
        assert refused("n_add=2^32", "2^32") and refused("n_add=SIZE_MAX", "2^32") and accepted("n_add=2^32-1")
        assert accepted("n_add=0") and accepted("n_add=0,d_add=NULL")
        for case in ("n_trees=SIZE_MAX/8/66+1", "n_trees=SIZE_MAX/64/bound+1", "n_trees*n_add>SIZE_MAX/2"):
            assert refused(case, "size overflow"), case
        for buf in ("tag", "d_counts", "d_frontier", "d_roots", "d_add", "d_add_offsets"):
            assert refused(buf + "=NULL", "NULL buffer"), buf
        for o in STATE:
            for i in INPUTS:
                assert refused("%s=%s+last" % (o, i), "%s overlaps %s" % (o, i)), (o, i)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
        # the witness buffers: NULL, misaligned, D == 0, k == 0
        for buf in IDS + MINE[:4]:
            assert refused(buf + "=NULL", "NULL buffer"), buf
        assert accepted("d_n_bad=NULL") and accepted("d_n_hashed=NULL") and accepted("d_n_bad_witness=NULL")
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 12 and all(refused(c, "aligned") for c in misaligned)
        assert {"d_wit_tree_ids+2", "d_wit_leaf_ids+4", "d_wit_leaves+8", "d_wit_siblings+8", "d_n_bad_witness+2"} <= set(misaligned)
        assert accepted("max_leaves=1,d_wit_siblings=NULL,d_wit_positions=NULL")
        assert refused("max_leaves=2,d_wit_siblings=NULL", "NULL buffer") and refused("max_leaves=2,d_wit_positions=NULL", "NULL buffer")
        for case in ("k=0", "k=0,witness=NULL", "k=0,d_wit_leaves+8", "k=0,d_wit_leaves=d_add"):
            assert accepted(case), case
        # the sizes
        for case in ("k=SIZE_MAX/128/D+1", "k=SIZE_MAX", "k=(256/D)*(2^31-1)+1", "max_leaves=1,k=256*(2^31-1)+1"):
            assert refused(case, "size overflow"), case
        assert accepted("k=(256/D)*(2^31-1)") and accepted("max_leaves=1,k=256*(2^31-1)")
        # every output of the pass against everything else, on both sides of its end
        n_pairs = 0
        for o in MINE:
            for i in STATE + INPUTS + IDS + tuple(x for x in MINE if x != o):
                row = by["%s=%s+last" % (o, i)]
                assert row[0] == -3 and "overlaps" in row[1] and o in row[1] and i in row[1], (o, i, row)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
                n_pairs += 1
        assert n_pairs == 5 * 13
        assert refused("d_wit_siblings=d_add-bytes+16", "d_wit_siblings overlaps d_add") and accepted("d_wit_siblings=d_add-bytes")


# ---- the kernel ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_witness.hip", os.path.join(CSRC, "_gen", "forest_witness_test.s"))


def test_the_one_kernel_uses_no_private_memory(compiled):
    res, isa = compiled
    assert len(res) == 2 and all("k_fw_refresh" in n for n in res), sorted(res)  # the one kernel, once per arity
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_the_unit_hashes_nothing_and_the_append_calls_it_once():
    from poseidon252_amd import build as b
    assert "forest_witness.hip" in b.SOURCES and "forest_witness.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_witness.hip")).read()
    for word in ("hades_permute", "node_digest_coop", "__shared__", "asm"):
        assert word not in src, word
    assert re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src) == ["k_fw_refresh"]
    assert "blockops.hpp" not in src and "while (lo < hi)" not in src and "for (unsigned off = 1; off <" not in src
    # both entry points go through one launcher, and the pass stands between the last digest launch and the state's update
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "forest_frontier.hip")).read())
    body = unit[unit.index("hipError_t launch_forest_frontier_append"):unit.index("hipError_t launch_forest_frontier_extract")]
    last = body.rindex("launch_forest_witness_refresh")
    assert body.rindex("launch_multiproof_digest_list") < last < body.index("k_ff_finish")
    assert "k_fw_" not in unit
    api = open(os.path.join(CSRC, "api.cpp")).read() + open(os.path.join(CSRC, "api_forest.cpp")).read()  # the host ABI, both files
    assert api.count("launch_forest_frontier_append(") == 2 and "launch_forest_witness_refresh" not in api


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    n_trees, max_leaves, n_add, k = 3, 100, 8, 5
    stride, D = FF.bound(max_leaves, arity), TS.depth(max_leaves, arity)
    args = dict(d_counts=dev(), d_frontier=dev(n=n_trees * stride * 4), d_roots=dev(), d_add=dev(n=n_add * 4), d_add_offsets=dev(),
                d_wit_tree_ids=dev(i32), d_wit_leaf_ids=dev(), d_wit_leaves=dev(n=k * 4), d_wit_siblings=dev(n=k * D * (arity - 1) * 4),
                d_wit_positions=dev(u8, n=k * D), d_wit_depths=dev(u8, n=k), d_n_bad=dev(i32), d_n_hashed=dev(), d_n_bad_witness=dev(i32))
    method = ctx.merkle4_forest_frontier_append_witness_device if arity == 4 else ctx.merkle2_forest_frontier_append_witness_device

    def call(a, k=k, max_leaves=max_leaves):
        return method(tag, a["d_counts"], a["d_frontier"], a["d_roots"], n_trees, max_leaves, a["d_add"], a["d_add_offsets"], a["d_wit_tree_ids"],
                      a["d_wit_leaf_ids"], k, a["d_wit_leaves"], a["d_wit_siblings"], a["d_wit_positions"], a["d_wit_depths"], a["d_n_bad"],
                      a["d_n_hashed"], a["d_n_bad_witness"])
    symbol = "p252_merkle%d_forest_frontier_append_witness_device_into" % arity
    call(args)
    assert recorder.calls == [symbol]  # the control: the library is reached, once, under this arity's symbol
    del recorder.calls[:]
    n_refused = 0
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match=where + " is on cpu"):
            call(bad)
        n_refused += 1
    assert n_refused == 14 and recorder.calls == []
    for name, short in (("d_counts", dev(n=n_trees - 1)), ("d_frontier", dev(n=n_trees * stride * 4 - 1)), ("d_roots", dev(n=n_trees * 4 - 1)),
                        ("d_add_offsets", dev(n=n_trees)), ("d_wit_tree_ids", dev(i32, n=k - 1)), ("d_wit_leaf_ids", dev(n=k - 1)),
                        ("d_wit_leaves", dev(n=k * 4 - 1)), ("d_wit_siblings", dev(n=k * D * (arity - 1) * 4 - 1)),
                        ("d_wit_positions", dev(u8, n=k * D - 1)), ("d_wit_depths", dev(u8, n=k - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call(dict(args, **{name: short}))
    for name, elem in (("d_counts", 8), ("d_add_offsets", 8), ("d_n_hashed", 8), ("d_wit_leaf_ids", 8), ("d_wit_positions", 1), ("d_wit_depths", 1)):
        with pytest.raises(ValueError, match="%s needs %d-byte elements" % (name, elem)):
            call(dict(args, **{name: dev(i32)}))
    for name in ("d_wit_tree_ids", "d_n_bad_witness"):
        with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
            call(dict(args, **{name: dev()}))
    with pytest.raises(ValueError, match="d_wit_siblings must be a torch tensor"):  # (only D == 0 has no rows)
        call(dict(args, d_wit_siblings=None))
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
    none = dict(args, d_add=None, d_wit_tree_ids=None, d_wit_leaf_ids=None, d_wit_leaves=None, d_wit_siblings=None, d_wit_positions=None,
                d_wit_depths=None, d_n_bad=None, d_n_hashed=None, d_n_bad_witness=None)
    call(none, k=0)
    call(dict(args, d_wit_siblings=None, d_wit_positions=None), max_leaves=1)
    a, b, c = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert a[2:] == (ptr(args["d_counts"]), ptr(args["d_frontier"]), ptr(args["d_roots"]), n_trees, max_leaves, ptr(args["d_add"]), n_add,
                     ptr(args["d_add_offsets"]), ptr(args["d_wit_tree_ids"]), ptr(args["d_wit_leaf_ids"]), k, ptr(args["d_wit_leaves"]),
                     ptr(args["d_wit_siblings"]), ptr(args["d_wit_positions"]), ptr(args["d_wit_depths"]), ptr(args["d_n_bad"]),
                     ptr(args["d_n_hashed"]), ptr(args["d_n_bad_witness"]), 0)
    assert b[7:] == (None, 0, ptr(args["d_add_offsets"]), None, None, 0, None, None, None, None, None, None, None, 0)
    assert c[5:7] == (n_trees, 1) and c[12:17] == (k, ptr(args["d_wit_leaves"]), None, None, ptr(args["d_wit_depths"]))


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_witness_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_witness_bench")
