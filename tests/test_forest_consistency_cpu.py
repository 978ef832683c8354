"""Consistency proofs of a ragged forest — that a grown tree extends its old root (p252_merkle{4,2}_forest_ragged_consistency_device_into
and _forest_consistency_verify_device_into; csrc/forest_consistency.hip) — what can be checked without a GPU: the numpy model the GPU
tests compare the calls with (testsupport/forestconsistency.py) against the oracle's builds for every pair of small counts, honest and
forked; the symbols declared, exported and mirrored; the host refusals as a table; the C++ mirror; the kernels' resources; the
Python methods validate every buffer before the library is reached."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
from testsupport import forestconsistency as FC  # noqa: E402
from testsupport import forestfrontier as FF  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_ragged_consistency_device_into": 17, "p252_merkle2_forest_ragged_consistency_device_into": 17,
           "p252_merkle4_forest_consistency_verify_device_into": 19, "p252_merkle2_forest_consistency_verify_device_into": 19}
TOP = {4: 70, 2: 40}  # every 1 <= n <= m <= TOP[arity]
MAX_LEAVES = {4: 1024, 2: 128}  # the stride exceeds every depth
FORK_TOP = 20


def _tag(arity):
    from poseidon252_amd import merkle
    return merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()


def _tree(oracle_mod, arity):
    return oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree


def _root(built, leaves, n):
    return FF.reduce_leaf(leaves[0]) if n == 1 else built[n][0]


# ---- the model against the oracle ----
@pytest.fixture(scope="module")
def builds(oracle_mod):
    """per arity: the leaves, and (root, levels) of the oracle's build of their first n, n = 1 .. TOP — computed once"""
    out = {}
    for arity in (4, 2):
        leaves = oracle_mod.fill_random(0xC50 + arity, TOP[arity])
        out[arity] = (leaves, {n: _tree(oracle_mod, arity)(_tag(arity), leaves[:n], want_levels=True)[:2] for n in range(1, TOP[arity] + 1)})
    return out


@pytest.mark.parametrize("arity", [4, 2])
def test_model_verifies_every_pair_against_the_oracles_builds(oracle_mod, builds, arity):
    """every 1 <= n <= m <= 70 (arity 2: 40): the old root from the left siblings alone is the oracle's root of leaves[:n], the new root
    its root of leaves[:m], the left siblings are frontier_of at n, the digests computed are the formula's; n = 1, A^d - 1, A^d, A^d + 1
    and m - n = 0 are all among them"""
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES[arity], arity)
    final_old_roots, grown = 0, []
    for m in range(1, TOP[arity] + 1):
        for n in range(1, m + 1):
            proof, new_count = FC.proof_of(leaves, built[m][1], m, n, arity, D)
            want_old, want_new = _root(built, leaves, n), _root(built, leaves, m)
            ok, old, new, hashed = FC.verify(proof, n, want_old, m, want_new, digest, arity)
            assert ok == 1 and new_count == m and proof.depth == TS.depth(m, arity), (arity, n, m)
            assert np.array_equal(old, want_old) and np.array_equal(new, want_new), (arity, n, m)
            assert hashed == FC.n_hashed(n, m, arity), (arity, n, m)
            if n < m:
                assert np.array_equal(FC.left_rows(proof, n, arity), FF.frontier_of(leaves[:n], built[n][1], n, arity, MAX_LEAVES[arity])), (arity, n, m)
                assert np.array_equal(proof.positions[:proof.depth], FC.digits(n, arity, proof.depth)), (arity, n, m)
                final_old_roots += n == arity ** TS.depth(n, arity)
                grown.append((proof.leaf, proof.siblings, n, m, old, new, hashed))
            else:
                assert not proof.leaf.any() and not proof.siblings.any() and not proof.positions.any() and hashed == 0
    assert final_old_roots > 100
    # the level-by-level form of the two chains (what the GPU tests use for thousands of proofs) gives the same roots and count
    many_old, many_new, many_hashed = FC.roots_many(np.array([g[0] for g in grown]), np.array([g[1] for g in grown]), [g[2] for g in grown],
                                                    [g[3] for g in grown], digest, arity)
    assert np.array_equal(many_old, np.array([g[4] for g in grown])) and np.array_equal(many_new, np.array([g[5] for g in grown]))
    assert many_hashed == sum(g[6] for g in grown)
    # the formula, by hand: 2 = 1 * A^0 + ... ; a power of the arity hashes nothing for the old side
    assert FC.n_hashed(1, 2, arity) == 1 and FC.n_hashed(arity, arity + 1, arity) == 2 and FC.n_hashed(5, 5, arity) == 0
    assert FC.old_digests(arity + 1, arity) == 2 and FC.old_digests(arity ** 2 + arity, arity) == 2 and FC.old_digests(arity ** 3, arity) == 0


@pytest.mark.parametrize("arity", [4, 2])
def test_model_refuses_a_tree_whose_old_leaf_was_altered_before_it_grew(oracle_mod, builds, arity):
    """every n <= m <= 20 and j in {0, n - 1}: leaf j < n altered, then the tree built to m leaves and the proof cut out of it honestly;
    against the honest old root and the forked new root the verdict is 0"""
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES[arity], arity)
    other = oracle_mod.fill_random(0xC60 + arity, FORK_TOP)
    fork = {}  # (j, m) -> the forked leaves and (root, levels) of their build, computed once

    def forked_build(j, m):
        if (j, m) not in fork:
            forked = leaves[:m].copy()
            forked[j] = other[j]
            fork[(j, m)] = (forked, {m: _tree(oracle_mod, arity)(_tag(arity), forked, want_levels=True)[:2]})
        return fork[(j, m)]
    n_checked = 0
    for m in range(1, FORK_TOP + 1):
        for n in range(1, m + 1):
            for j in sorted({0, n - 1}):
                forked, fbuilt = forked_build(j, m)
                proof, _ = FC.proof_of(forked, fbuilt[m][1], m, n, arity, D)
                honest_old, forked_new = _root(built, leaves, n), _root(fbuilt, forked, m)
                ok, old, new, _ = FC.verify(proof, n, honest_old, m, forked_new, digest, arity)
                assert ok == 0, (arity, j, n, m)
                if n < m:  # the forked tree is consistent with ITS old root: only the honest one is refused
                    assert np.array_equal(new, forked_new) and not np.array_equal(old, honest_old), (arity, j, n, m)
                    assert FC.verify(proof, n, old, m, new, digest, arity)[0] == 1
                n_checked += 1
    assert n_checked == 2 * 210 - FORK_TOP  # (n == 1 has j = 0 only)


@pytest.mark.parametrize("arity", [4, 2])
def test_model_refusals_and_tampering(oracle_mod, builds, arity):
    leaves, built = builds[arity]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    D = TS.depth(MAX_LEAVES[arity], arity)
    n, m = 17, 37
    proof, _ = FC.proof_of(leaves, built[m][1], m, n, arity, D)
    old, new = built[n][0], built[m][0]
    assert FC.verify(proof, n, old, m, new, digest, arity)[0] == 1
    for bad_n, bad_m in ((0, m), (m + 1, m), (m, n)):
        ok, r_old, r_new, hashed = FC.verify(proof, bad_n, old, bad_m, new, digest, arity)
        assert ok == 0 and hashed == 0 and not r_old.any() and not r_new.any(), (bad_n, bad_m)
    for depth in (proof.depth - 1, proof.depth + 1, 0xFF):
        w = proof.copy()
        w.depth = depth
        assert FC.verify(w, n, old, m, new, digest, arity)[0] == 0
    w = proof.copy()
    w.positions[0] ^= 1
    assert FC.verify(w, n, old, m, new, digest, arity)[0] == 0
    w = proof.copy()
    w.siblings[TS.depth(m, arity)] ^= np.uint64(1)  # a row that is not read
    assert FC.verify(w, n, old, m, new, digest, arity)[0] == 1
    # the roots do not commit to a count beyond its depth: m + 1 passes where depth(m + 1) == depth(m), and only there
    assert TS.depth(m + 1, arity) == TS.depth(m, arity) and FC.verify(proof, n, old, m + 1, new, digest, arity)[0] == 1
    top = arity ** 2
    p2, _ = FC.proof_of(leaves, built[top][1], top, 3, arity, D)
    assert FC.verify(p2, 3, built[3][0], top, built[top][0], digest, arity)[0] == 1 and FC.verify(p2, 3, built[3][0], top + 1, built[top][0], digest, arity)[0] == 0
    # bad extractions
    for bad_n, bad_m in ((0, 5), (6, 5), (1, 0)):
        w, new_count = FC.proof_of(leaves, built[5][1], bad_m, bad_n, arity, D)
        assert w.bad() and new_count == 0 and not w.leaf.any() and not w.siblings.any()


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    raw, header = check_abi_symbols(SYMBOLS)
    listed = raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    assert "_forest_ragged_consistency_device_into" in listed and "_forest_consistency_verify_device_into" in listed
    assert not any("consistency" in s for s in re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("consistency_refusal_table", tmp_path_factory.mktemp("consistency_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "consistency_refusals")


EXTRACT_IN = ("d_leaves", "d_offsets", "d_levels", "d_tree_ids", "d_old_counts")
EXTRACT_OUT = ("d_new_counts_out", "d_leaves_out", "d_siblings", "d_positions", "d_depths", "d_n_bad")
VERIFY_IN = ("d_old_counts", "d_old_roots", "d_new_counts", "d_new_roots", "d_leaves_in", "d_siblings", "d_positions", "d_depths", "d_tree_ids")
VERIFY_OUT = ("d_ok", "d_old_roots_out", "d_new_roots_out", "d_n_hashed")


def _overlap_rows(by, ins, outs):
    refused = lambda case, a, b: by[case][0] == -3 and "overlaps" in by[case][1] and a in by[case][1] and b in by[case][1]  # noqa: E731
    n = 0
    for o in outs:
        for i in ins + tuple(x for x in outs if x != o):
            assert refused("%s=%s+last" % (o, i), o, i), (o, i, by["%s=%s+last" % (o, i)])
            assert by["%s=%s+end" % (o, i)] == by["control"], (o, i)
            n += 1
    return n


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_ragged_consistency_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and by["k=0"] == (0, "") and by["k=0,all=NULL,max_leaves=0"] == (0, "")
        for case in ("max_leaves=0", "n_trees=0", "n_leaves=0"):
            assert refused(case, "must be > 0"), case
        assert accepted("max_leaves=1,d_levels=NULL,d_siblings=NULL,d_positions=NULL") and accepted("max_leaves=SIZE_MAX")
        assert refused("max_leaves=2,d_siblings=NULL", "NULL buffer") and refused("max_leaves=2,d_positions=NULL", "NULL buffer")
        for case in ("n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "k=SIZE_MAX/128/D+1", "k=SIZE_MAX"):
            assert refused(case, "size overflow"), case
        for buf in EXTRACT_IN + EXTRACT_OUT[:5]:
            assert refused(buf + "=NULL", "NULL buffer"), buf
        assert accepted("d_n_bad=NULL")
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 9 and all(refused(c, "aligned") for c in misaligned)
        assert {"d_leaves+8", "d_offsets+4", "d_tree_ids+2", "d_old_counts+4", "d_new_counts_out+4", "d_siblings+8", "d_n_bad+2"} <= set(misaligned)
        assert _overlap_rows(by, EXTRACT_IN, EXTRACT_OUT) == 6 * 10
        assert refused("d_siblings=d_leaves-bytes+16", "d_siblings overlaps d_leaves") and accepted("d_siblings=d_leaves-bytes")

        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_consistency_verify_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")
        assert by["ctx=NULL"][0] == -3 and by["k=0"] == (0, "") and by["k=0,all=NULL,stride_depth=65"] == (0, "")
        assert refused("tag=NULL", "NULL buffer") and accepted("stride_depth=64")
        assert refused("stride_depth=65", "stride_depth must be <= 64") and refused("stride_depth=SIZE_MAX", "stride_depth must be <= 64")
        assert accepted("stride_depth=0,d_siblings=NULL,d_positions=NULL")
        # the claims: per proof without tree ids, per tree with them; a forest of no tree has none
        assert accepted("d_tree_ids=NULL") and accepted("d_tree_ids=NULL,n_trees=0") and accepted("n_trees=0,claims=NULL")
        assert refused("d_tree_ids=NULL,n_trees=0,d_old_roots=NULL", "NULL buffer")
        assert accepted("roots_out=NULL,d_n_hashed=NULL") and accepted("d_old_roots_out=NULL") and accepted("d_new_roots_out=NULL") and accepted("d_n_hashed=NULL")
        for buf in VERIFY_IN[:8] + ("d_ok",):
            assert refused(buf + "=NULL", "NULL buffer"), buf
        for case in ("n_trees=SIZE_MAX/64+1", "k=SIZE_MAX/128/D+1", "k=SIZE_MAX"):
            assert refused(case, "size overflow"), case
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 10 and all(refused(c, "aligned") for c in misaligned)
        assert {"d_old_counts+4", "d_old_roots+8", "d_new_counts+4", "d_new_roots+8", "d_leaves_in+8", "d_tree_ids+2", "d_n_hashed+4"} <= set(misaligned)
        assert _overlap_rows(by, VERIFY_IN, VERIFY_OUT) == 4 * 12
        assert refused("d_tree_ids=NULL,d_n_hashed=d_old_counts+24", "d_n_hashed overlaps d_old_counts") and accepted("d_n_hashed=d_old_counts+24")


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_consistency.hip", os.path.join(CSRC, "_gen", "forest_consistency_test.s"))


def test_the_units_kernels_keep_the_projects_resource_conditions(compiled):
    """no private memory, no AGPRs, at least two waves per SIMD (tests/test_kernel_resources.py's conditions) for the unit's three
    kernels — the record, the lay-out of the two walks (once per arity) and the verdicts; none of them hashes"""
    res, isa = compiled
    assert len([n for n in res if "k_fc_prepare" in n]) == 2
    assert len([n for n in res if "k_fc_record" in n]) == 1 and len([n for n in res if "k_fc_finish" in n]) == 1 and len(res) == 4, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["occ"] >= 2 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_the_unit_hashes_through_the_path_kernel_and_shares_the_extraction_and_the_sort():
    """every hashing kernel of the library has its row in the edge-value matrix (tests/edgecases.py); this unit adds none: both
    chains of a proof are walks of k_path_ragged, which the matrix names"""
    from poseidon252_amd import build as b
    import edgecases
    assert "forest_consistency.hip" in b.SOURCES and "forest_consistency.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_consistency.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src) == ["k_fc_record", "k_fc_prepare", "k_fc_finish"]
    for word in ("hades_permute", "node_digest_coop", "asm", "blockops.hpp", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy"):
        assert word not in code, word
    assert code.count("launch_path_ragged(") == 2 and "launch_forest_opening_pieces(" in code
    assert not re.search(r"\bk_(fo|fr|path)_\w+\s*[(<]", code)  # the neighbours' kernels through their launchers only
    assert set(edgecases.hashing_kernels()) <= set(edgecases.named_kernels()) and "k_path_ragged" in edgecases.named_kernels()
    api = open(os.path.join(CSRC, "api_forest.cpp")).read()
    body = api[api.index("static int forest_consistency_verify_device"):api.index("P252_MERKLE_PAIR(int, forest_ragged_consistency_device_into")]
    assert "ragged_sort_enabled()" in body and body.count("with_stream_scratch(") == 1 and "hipMalloc" not in body


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    n_trees, max_leaves, k = 3, 100, 5
    D = TS.depth(max_leaves, arity)
    extract = ctx.merkle4_forest_ragged_consistency_device if arity == 4 else ctx.merkle2_forest_ragged_consistency_device
    verify = ctx.merkle4_forest_consistency_verify_device if arity == 4 else ctx.merkle2_forest_consistency_verify_device
    e_args = dict(d_leaves=dev(n=120 * 4), d_offsets=dev(), d_levels=dev(n=(120 // (arity - 1) + n_trees * D) * 4), d_tree_ids=dev(i32), d_old_counts=dev(),
                  d_new_counts_out=dev(), d_leaves_out=dev(n=k * 4), d_siblings=dev(n=k * D * (arity - 1) * 4), d_positions=dev(u8, n=k * D),
                  d_depths=dev(u8, n=k), d_n_bad=dev(i32))
    v_args = dict(d_old_counts=dev(), d_old_roots=dev(n=k * 4), d_new_counts=dev(), d_new_roots=dev(n=k * 4), d_leaves=dev(n=k * 4),
                  d_siblings=dev(n=k * D * (arity - 1) * 4), d_positions=dev(u8, n=k * D), d_depths=dev(u8, n=k), d_ok=dev(u8, n=k), d_tree_ids=dev(i32),
                  d_old_roots_out=dev(n=k * 4), d_new_roots_out=dev(n=k * 4), d_n_hashed=dev())

    def call_e(a, k=k, max_leaves=max_leaves):
        return extract(a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_tree_ids"], a["d_old_counts"], k, a["d_new_counts_out"],
                       a["d_leaves_out"], a["d_siblings"], a["d_positions"], a["d_depths"], a["d_n_bad"])

    def call_v(a, k=k, stride=D, n_trees=n_trees):
        return verify(tag, a["d_old_counts"], a["d_old_roots"], a["d_new_counts"], a["d_new_roots"], a["d_leaves"], a["d_siblings"], a["d_positions"],
                      a["d_depths"], stride, k, a["d_ok"], a["d_tree_ids"], n_trees, a["d_old_roots_out"], a["d_new_roots_out"], a["d_n_hashed"])
    e_sym, v_sym = "p252_merkle%d_forest_ragged_consistency_device_into" % arity, "p252_merkle%d_forest_consistency_verify_device_into" % arity
    call_e(e_args), call_v(v_args)
    assert recorder.calls == [e_sym, v_sym]  # the control: the library is reached, once each, under this arity's symbols
    del recorder.calls[:]
    n_refused = 0
    for call, args in ((call_e, e_args), (call_v, v_args)):
        for where, bad in with_cpu_tensor(args):
            with pytest.raises(ValueError, match=where + " is on cpu"):
                call(bad)
            n_refused += 1
    assert n_refused == 11 + 13 and recorder.calls == []
    for name, short in (("d_offsets", dev(n=n_trees)), ("d_levels", dev(n=8)), ("d_tree_ids", dev(i32, n=k - 1)), ("d_old_counts", dev(n=k - 1)),
                        ("d_new_counts_out", dev(n=k - 1)), ("d_leaves_out", dev(n=k * 4 - 1)), ("d_siblings", dev(n=k * D * (arity - 1) * 4 - 1)),
                        ("d_positions", dev(u8, n=k * D - 1)), ("d_depths", dev(u8, n=k - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call_e(dict(e_args, **{name: short}))
    for name, short in (("d_old_counts", dev(n=n_trees - 1)), ("d_old_roots", dev(n=n_trees * 4 - 1)), ("d_new_counts", dev(n=n_trees - 1)),
                        ("d_new_roots", dev(n=n_trees * 4 - 1)), ("d_leaves", dev(n=k * 4 - 1)), ("d_siblings", dev(n=k * D * (arity - 1) * 4 - 1)),
                        ("d_positions", dev(u8, n=k * D - 1)), ("d_depths", dev(u8, n=k - 1)), ("d_ok", dev(u8, n=k - 1)), ("d_tree_ids", dev(i32, n=k - 1)),
                        ("d_old_roots_out", dev(n=k * 4 - 1)), ("d_new_roots_out", dev(n=k * 4 - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call_v(dict(v_args, **{name: short}))
    with pytest.raises(ValueError, match="d_old_counts holds"):  # without tree ids the claims are per proof
        call_v(dict(v_args, d_tree_ids=None, d_old_counts=dev(n=k - 1)))
    for call, args, names in ((call_e, e_args, (("d_offsets", 8), ("d_old_counts", 8), ("d_new_counts_out", 8), ("d_positions", 1), ("d_depths", 1))),
                              (call_v, v_args, (("d_old_counts", 8), ("d_new_counts", 8), ("d_n_hashed", 8), ("d_positions", 1), ("d_depths", 1), ("d_ok", 1)))):
        for name, elem in names:
            with pytest.raises(ValueError, match="%s needs %d-byte elements" % (name, elem)):
                call(dict(args, **{name: dev(i32)}))
    for call, args, name in ((call_e, e_args, "d_tree_ids"), (call_e, e_args, "d_n_bad"), (call_v, v_args, "d_tree_ids")):
        with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
            call(dict(args, **{name: dev()}))
    with pytest.raises(ValueError, match="d_siblings must be a torch tensor"):  # (only D == 0 has no rows)
        call_e(dict(e_args, d_siblings=None))
    with pytest.raises(ValueError, match="stride_depth must be in 0 .. 64"):
        call_v(v_args, stride=65)
    assert recorder.calls == []
    assert "arity" not in __import__("inspect").signature(extract).parameters and "arity" not in __import__("inspect").signature(verify).parameters
    # the sizes the C calls receive
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name in (e_sym, v_sym):
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    call_e(e_args)
    call_e(dict(e_args, d_levels=None, d_siblings=None, d_positions=None, d_n_bad=None), max_leaves=1)
    call_v(v_args)
    call_v(dict(v_args, d_tree_ids=None, d_old_roots_out=None, d_new_roots_out=None, d_n_hashed=None, d_siblings=None, d_positions=None), stride=0, n_trees=0)
    a, b, c, d = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert a[1:] == (ptr(e_args["d_leaves"]), 120, ptr(e_args["d_offsets"]), n_trees, max_leaves, ptr(e_args["d_levels"]), ptr(e_args["d_tree_ids"]),
                     ptr(e_args["d_old_counts"]), k, ptr(e_args["d_new_counts_out"]), ptr(e_args["d_leaves_out"]), ptr(e_args["d_siblings"]),
                     ptr(e_args["d_positions"]), ptr(e_args["d_depths"]), ptr(e_args["d_n_bad"]), 0)
    assert b[5:7] == (1, None) and b[12:] == (None, None, ptr(e_args["d_depths"]), None, 0)
    assert c[2:] == (ptr(v_args["d_old_counts"]), ptr(v_args["d_old_roots"]), ptr(v_args["d_new_counts"]), ptr(v_args["d_new_roots"]),
                     ptr(v_args["d_leaves"]), ptr(v_args["d_siblings"]), ptr(v_args["d_positions"]), ptr(v_args["d_depths"]), D, k,
                     ptr(v_args["d_tree_ids"]), n_trees, ptr(v_args["d_ok"]), ptr(v_args["d_old_roots_out"]), ptr(v_args["d_new_roots_out"]),
                     ptr(v_args["d_n_hashed"]), 0)
    assert d[7:9] == (None, None) and d[10:] == (0, k, None, 0, ptr(v_args["d_ok"]), None, None, None, 0)


def test_the_helpers_are_exported():
    import poseidon252_amd as P
    assert callable(P.forest_ragged_consistency) and callable(P.forest_consistency_verify)
    assert {"forest_ragged_consistency", "forest_consistency_verify"} <= set(P.__all__)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_consistency_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_consistency_bench")
