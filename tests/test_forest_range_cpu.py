"""Whole runs of leaves of a ragged forest proved and checked in one call (p252_merkle{4,2}_forest_ragged_range_proofs_device_into /
p252_merkle{4,2}_forest_range_verify_device_into; csrc/forest_range.hip) — what can be checked without a GPU: the numpy model the GPU
tests compare the calls with (testsupport/forestrange.py) against the model of the shared proof for the same positions, for EVERY run
of every tree of up to 40 leaves, and against the oracle's roots; the stride, the host's level bound and the dense packing; the symbols
declared, exported and mirrored; the host refusals as a table; the kernels' resources; the Python methods."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
import edgecases as E  # noqa: E402
from testsupport import forestrange as FR  # noqa: E402
from testsupport import multiproofmodel as MP  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table  # noqa: E402

SYMBOLS = {"p252_merkle4_forest_ragged_range_proofs_device_into": 18, "p252_merkle2_forest_ragged_range_proofs_device_into": 18,
           "p252_merkle4_forest_range_verify_device_into": 20, "p252_merkle2_forest_range_verify_device_into": 20}


def _tag(arity):
    from poseidon252_amd import merkle
    return merkle.merkle4_tag() if arity == 4 else merkle.merkle2_tag()


# ---- the model against the model of the shared proof ----
@pytest.mark.parametrize("arity", [4, 2])
def test_model_equals_the_shared_proof_of_the_same_positions_for_every_run(arity):
    """every (n, a, b) with n <= 40: proof nodes, S_l and both counts equal multiproofmodel's for positions = arange(a, b); the stride
    holds every proof"""
    n_runs, fill = 0, 0.0
    for n in range(1, 41):
        stride = FR.range_stride(n, arity)
        assert stride == 2 * (arity - 1) * TS.depth(n, arity)
        for a in range(n):
            for b in range(a + 1, n + 1):
                nodes, S, w = FR.range_model(n, a, b, arity)
                m_nodes, m_S, m_w = MP.multiproof_model(n, np.arange(a, b), arity)
                assert w == m_w and len(nodes) == len(m_nodes) == TS.depth(n, arity), (n, a, b)
                assert all(np.array_equal(x, y) for x, y in zip(nodes, m_nodes)), (n, a, b)
                assert all(np.array_equal(np.arange(lo, hi), y) for (lo, hi), y in zip(S, m_S)), (n, a, b)
                length, digests = FR.range_counts(n, a, b, arity)
                assert (length, digests) == MP.multiproof_counts(n, np.arange(a, b), arity)
                assert length <= stride and all(p.size <= 2 * (arity - 1) for p in nodes)
                fill = max(fill, length / stride if stride else 0.0)
                n_runs += 1
        assert FR.range_counts(n, 0, n, arity) == (0, TS.levels_len(n, arity))  # a whole tree: no proof, every node hashed
    print("arity %d: %d runs, the fullest row %.3f of the stride" % (arity, n_runs, fill))
    assert n_runs == sum(n * (n + 1) // 2 for n in range(1, 41)) and 0.5 < fill <= 1.0


@pytest.mark.parametrize("arity", [4, 2])
def test_models_proofs_re_hash_to_the_oracles_roots(oracle_mod, arity):
    """the model's extraction out of the oracle's trees: the single-tree verifier's model (multiproof_root) and this model's own
    re-hash both give the oracle's root, for every run of trees around the powers of the arity"""
    tag = _tag(arity)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    digest = lambda kids: oracle_mod.hash_batch(tag, kids, arity, 1)  # noqa: E731
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33]
    leaves = oracle_mod.fill_random(0xA11 + arity, sum(sizes))
    off = TS.offsets(sizes, dtype=np.int64)
    built = [tree(tag, leaves[off[t]:off[t + 1]], want_levels=True)[:2] for t in range(len(sizes))]
    levels = np.concatenate([np.asarray(lv).reshape(-1, 4) for _, lv in built])
    runs = [(t, a, b - a) for t, n in enumerate(sizes) for a in range(n) for b in range(a + 1, n + 1)]
    tid, first, lens = (np.array([r[c] for r in runs]) for c in range(3))
    loff = TS.offsets(lens)
    k, top = int(loff[-1]), max(sizes)
    proof, plen, counts, out, bad = FR.range_extract(leaves, off, levels, tid, first, loff, k, top, arity)
    assert bad == 0 and np.array_equal(counts, np.asarray(sizes)[tid].astype(np.uint64))
    for r in range(0, len(runs), 3):
        t, a, n = runs[r]
        vals = out[int(loff[r]):int(loff[r + 1])]
        want = E.reduce_mod_p(leaves[off[t]:off[t] + 1])[0] if sizes[t] == 1 else built[t][0]
        assert np.array_equal(vals, leaves[off[t] + a:off[t] + a + n])
        got = MP.multiproof_root(sizes[t], np.arange(a, a + n), vals, proof[r, :int(plen[r])], arity, digest)
        mine = FR.range_root(sizes[t], a, vals, proof[r], arity, digest)
        assert not proof[r, int(plen[r]):].any()
        if sizes[t] > 1:
            assert np.array_equal(got, want) and np.array_equal(mine, want), (sizes[t], a, n)
    # the verdicts of the whole batch, and of one with a changed leaf, a short row and a claimed count that moves no width
    ok, roots_out, hashed, bad = FR.range_verify(counts, tid, first, loff, k, top, out, proof, plen, np.stack([E.reduce_mod_p(leaves[:1])[0]] + [b[0] for b in built[1:]]),
                                                 arity, digest, E.reduce_mod_p)
    assert ok.all() and bad == 0 and hashed == sum(FR.range_counts(sizes[t], a, a + n, arity)[1] for t, a, n in runs)


# ---- the bad-run rule ----
def test_run_lengths_follow_the_ragged_forests_rule_for_offsets():
    assert FR.run_lengths([0, 3, 3, 10], 10).tolist() == [3, 0, 7]  # no leaf
    assert FR.run_lengths([0, 3, 2, 10], 10).tolist() == [3, 0, 0]  # decreasing; then the lengths before run 2 and its own pass k
    assert FR.run_lengths([0, 3, 2, 9], 10).tolist() == [3, 0, 7]
    assert FR.run_lengths([0, 3, 11], 10).tolist() == [3, 0]  # past k
    assert FR.run_lengths([0, 6, 3, 9], 10).tolist() == [6, 0, 0]  # 6 + 6 > 10
    assert FR.run_lengths([2 ** 64 - 2, 2 ** 64 - 1], 10).tolist() == [0]
    good, lens = FR.good_runs([5, 5, 5, 5, 0, 5], [0, 0, 7, 0, 0, 0], [0, 2, 0, 5, 0, 2 ** 64 - 1], TS.offsets([5, 3, 1, 1, 1, 2]), 13, 7, 5)
    assert good.tolist() == [True, True, False, False, False, False] and lens.tolist() == [5, 3, 1, 1, 1, 2]
    good, _ = FR.good_runs([6, 1], [0, 1], [0, 0], TS.offsets([2, 1]), 3, 2, 5)  # a count above max_leaves
    assert good.tolist() == [False, True]


# ---- the host's bound of a level, and the dense packing ----
@pytest.mark.parametrize("arity", [4, 2])
def test_level_bound_holds_and_the_dense_lists_have_no_gap(arity):
    rng = np.random.default_rng(arity)
    tight = 0.0
    for trial in range(300):
        m = int(rng.integers(1, 40))
        top = int(rng.choice([3, 17, 70, 1000, 5000]))
        counts = rng.integers(1, top + 1, size=m)
        first = np.array([rng.integers(0, n) for n in counts])
        lens = np.array([rng.integers(1, min(n - a, 1 + 3 * trial % 50) + 1) for n, a in zip(counts, first)])
        counts[rng.random(m) < 0.1] = 0  # runs that take no part
        D = int(TS.depth(top, arity))
        k = int(lens.sum()) + int(rng.integers(0, 3))
        base, totals = FR.scan_bases(counts, first, lens, D, arity)
        assert base.shape == (D + 1, m) and not base[:, 0].any()
        for l in range(D + 1):
            cnt = [0 if not counts[r] or l > TS.depth(int(counts[r]), arity) else FR.range_model(int(counts[r]), int(first[r]), int(first[r] + lens[r]), arity)[1][l]
                   for r in range(m)]
            cnt = [c if c == 0 else c[1] - c[0] for c in cnt]
            assert np.array_equal(np.diff(np.append(base[l], totals[l])), cnt)  # gap-free: every run's nodes follow the run's before it
            if l:
                assert totals[l] <= FR.level_bound(k, m, l, arity), (arity, trial, l)
                tight = max(tight, totals[l] / FR.level_bound(k, m, l, arity))
        assert totals[0] <= k
    # the bound is reached: runs of one leaf at odd places have two... one node a level each, runs across a parent's border two
    assert tight > 0.6
    assert FR.level_bound(10, 3, 1, arity) == min(13, 10 // arity + 6) and FR.level_bound(1 << 20, 1, 1, arity) == (1 << 20) // arity + 2


# ---- the symbols ----
def test_symbols_declared_exported_and_in_sys_rs():
    from poseidon252_amd import _lib
    raw, header = check_abi_symbols(SYMBOLS)
    listed = raw.split("#define P252_ABI_VERSION")[0]  # the ABI-9 list names them
    for name in ("_forest_range_stride", "_forest_ragged_range_proofs_device_into", "_forest_range_verify_device_into"):
        assert name in listed, name
    assert not any("range" in s for s in re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))  # (api_refusals.cpp's table stays as it is)
    for arity in (4, 2):
        name = "p252_merkle%d_forest_range_stride" % arity
        assert re.search(r"\bsize_t %s\s*\(size_t max_leaves\);" % name, header) and name in _lib.ABI_SYMBOLS
        assert _lib.PROTOTYPES[name] == ([_lib._sz], _lib._sz)
        for n in (1, 2, 5, 100, 257, 2 ** 32 - 1):
            assert getattr(_lib.lib(), name)(n) == FR.range_stride(n, arity)
    doc = raw[raw.index("/* ---- runs:"):raw.index("int p252_merkle4_forest_range_verify_device_into")]
    for word in ("p252_trim", "0xFFFFFFFF", "multiproof_device", "byte for byte", "mod p", "bytes a run"):
        assert word in doc, word
    # the order of _lib.PROTOTYPES is the header's
    order = [n for n in re.findall(r"\b(p252_\w+)\s*\(", header) if n in _lib.PROTOTYPES]
    assert list(dict.fromkeys(order)) == list(_lib.PROTOTYPES)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    n_rust = len(re.findall(r"pub fn p252_", open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()))
    assert "(%d functions" % n_rust in integration


def test_the_helpers_are_exported_and_no_arity_method_is_added():
    import poseidon252_amd as P
    from poseidon252_amd import Context, hash as H
    for name in ("forest_ragged_range_proofs", "forest_range_verify", "forest_range_stride"):
        assert callable(getattr(P, name)) and name in P.__all__, name
        assert inspect.signature(getattr(P, name)).parameters["arity"].default == 4
    for stem in ("forest_ragged_range_proofs_device", "forest_range_verify_device"):
        assert not hasattr(Context, "merkle_" + stem) and stem not in H._PER_ARITY_STEMS
        for arity in (4, 2):
            m = getattr(Context, "merkle%d_%s" % (arity, stem))
            assert inspect.isfunction(m) and m.__name__ == "merkle%d_%s" % (arity, stem) and "arity" not in inspect.signature(m).parameters
            assert "p252_merkle%d_" % arity in m.__doc__


# ---- the host refusals ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("range_refusal_table", tmp_path_factory.mktemp("range_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "range_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        strides = {r[1]: r[2] for r in table if r[0] == "p252_merkle%d_forest_range_stride" % arity}
        assert strides["max_leaves=0"] == 0 == strides["max_leaves=1"] and strides["max_leaves=100"] == FR.range_stride(100, arity)
        for which, sym in enumerate(("p252_merkle%d_forest_ragged_range_proofs_device_into", "p252_merkle%d_forest_range_verify_device_into")):
            by = {r[1]: r[2:] for r in table if r[0] == sym % arity}
            assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
            refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
            accepted = lambda case: by[case] == by["control"]  # noqa: E731
            assert by["ctx=NULL"][0] == -3
            for case in ("m=0", "k=0", "n_trees=0", "max_leaves=0"):
                assert refused(case, "must be > 0"), case
            for case in ("k=2^32", "k=SIZE_MAX", "m=2^32", "m=SIZE_MAX", "max_leaves=2^32", "max_leaves=SIZE_MAX", "k+2m=2^32", "k=2^32-1", "m=2^31"):
                assert refused(case, "below 2^32"), case
            assert accepted("k+2m=2^32-1") and accepted("m=2^31-5,k+2m=2^32-1") and accepted("max_leaves=2^32-1") and accepted("counters=NULL")
            nulls = [c for c in by if re.fullmatch(r"d_\w+=NULL", c)]
            optional = {"d_n_bad=NULL", "d_leaves_out=NULL"} if which == 0 else {"d_n_bad=NULL", "d_n_hashed=NULL", "d_roots_out=NULL"}
            assert len(nulls) == (11, 12)[which]
            for c in nulls:
                assert accepted(c) if c in optional else refused(c, "NULL buffer"), c
            misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
            assert len(misaligned) == (11, 11)[which] and all(refused(c, "aligned") for c in misaligned)
            if which == 0:
                assert refused("n_leaves=0", "must be > 0") and accepted("max_leaves=1,d_levels=NULL,d_proof=NULL")
                assert refused("max_leaves=2,d_levels=NULL", "NULL buffer") and refused("max_leaves=2,d_proof=NULL", "NULL buffer")
                for case in ("n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "n_trees*min(max_leaves,n_leaves)>SIZE_MAX/2"):
                    assert refused(case, "size overflow"), case
            else:
                assert refused("tag=NULL", "NULL buffer") and accepted("proof_stride=0,d_proof=NULL") and accepted("proof_stride=1000")
                assert accepted("m*proof_stride=SIZE_MAX>>8") and accepted("n_trees=SIZE_MAX/32")
                for case in ("m*proof_stride>SIZE_MAX>>8", "proof_stride=SIZE_MAX", "n_trees=SIZE_MAX/32+1"):
                    assert refused(case, "size overflow"), case


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_range.hip", os.path.join(CSRC, "_gen", "forest_range_test.s"))


def test_the_units_kernels_move_data_in_32_registers_and_no_private_memory(compiled):
    """no private memory, no AGPRs and at most 32 VGPRs for every kernel of the unit: the check, the gather, the leaf move, the records,
    the one-leaf roots and the finish (the check, the gather and the records once per arity); none of them hashes"""
    res, isa = compiled
    for one, n in (("k_rg_check", 2), ("k_rg_gather", 2), ("k_rg_records", 2), ("k_rg_move", 1), ("k_rg_leaf_roots", 1), ("k_rg_finish", 1)):
        assert len([name for name in res if one in name]) == n, one
    assert len(res) == 9, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 32 and v["occ"] >= 8, (name, v)
    assert "scratch_" not in isa
    gather = isa[isa.index("k_rg_gather"):]
    assert "global_load_dwordx4" in gather and "global_store_dwordx4" in gather  # 32 bytes as two 16-byte accesses


def test_the_unit_hashes_through_the_multiproofs_digest_launch_and_the_streams_scratch():
    """every hashing kernel of the library has its row in the edge-value matrix (tests/edgecases.py); this unit adds none: the digests
    go through launch_multiproof_digest_list.  The index of the forest and of the runs and the scan of the runs' node counts are the
    ragged forest's own launchers (whose kernels use the shared scan primitives of blockops.hpp); the scratch is the stream's pair;
    nothing is allocated and nothing waits."""
    from poseidon252_amd import build as b
    assert "forest_range.hip" in b.SOURCES and "forest_range.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_range.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    mine = set(re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src))
    assert mine == {"k_rg_check", "k_rg_gather", "k_rg_move", "k_rg_records", "k_rg_leaf_roots", "k_rg_finish"}
    assert not (E.hashing_kernels() & mine) and set(E.hashing_kernels()) <= set(E.named_kernels())
    for word in ("hades_permute", "node_digest_coop", "asm", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "atomicCAS"):
        assert word not in code, word
    assert code.count("launch_multiproof_digest_list(") == 1 and code.count("launch_forest_ragged_index(") == 1
    assert code.count("launch_forest_scan_rows(") == 2  # the leaves' row of the extraction, the levels' rows of the verification
    ragged = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "forest_ragged.hip")).read())
    rows_scan = ragged[ragged.index("hipError_t launch_forest_scan_rows("):ragged.index("hipError_t launch_forest_ragged(")]
    assert rows_scan.count("hipLaunchKernelGGL(") == 3 and "k_fr_scan_tiles" in rows_scan  # three launches for all levels at once
    assert "block_exclusive<" in ragged[ragged.index("k_fr_rows_tile_sums"):ragged.index("k_fr_block_first")]
    assert not re.search(r"\bk_(fm|mp|fr|fo)_\w+\s*[(<]", code)  # the neighbours' kernels through their launchers only
    api = open(os.path.join(CSRC, "api_forest.cpp")).read()
    extract = api[api.index("static int forest_ragged_range_proofs_device"):api.index("static int forest_range_verify_device")]
    verify = api[api.index("static int forest_range_verify_device"):api.index("P252_MERKLE_PAIR(int, forest_ragged_range_proofs_device_into")]
    assert extract.count("with_forest_index(") == 1 and "with_stream_scratch(" not in extract and "forest_shape_check(" in extract
    assert verify.count("with_stream_scratch(") == 1 and "with_forest_index(" not in verify
    for body in (extract, verify):
        assert "forest_range_shape_check(" in body and "hipMalloc" not in body and "Synchronize" not in body


# ---- the Python methods ----
@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_cpu_tensors_and_pass_the_sizes(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    n_trees, max_leaves, m, k = 3, 100, 4, 9
    D = TS.depth(max_leaves, arity)
    P = FR.range_stride(max_leaves, arity)
    extract = getattr(ctx, "merkle%d_forest_ragged_range_proofs_device" % arity)
    verify = getattr(ctx, "merkle%d_forest_range_verify_device" % arity)
    args = dict(d_leaves=dev(n=120 * 4), d_offsets=dev(), d_levels=dev(n=(120 // (arity - 1) + n_trees * D) * 4), d_tree_ids=dev(i32), d_first=dev(),
                d_leaf_offsets=dev(n=m + 1), d_proof=dev(n=m * P * 4), d_proof_lens=dev(i32), d_counts=dev(), d_leaves_out=dev(n=k * 4), d_n_bad=dev(i32),
                d_roots=dev(n=n_trees * 4), d_ok=dev(u8, n=m), d_roots_out=dev(n=m * 4), d_n_hashed=dev())

    def call_e(a, max_leaves=max_leaves):
        return extract(a["d_leaves"], a["d_offsets"], n_trees, max_leaves, a["d_levels"], a["d_tree_ids"], a["d_first"], a["d_leaf_offsets"], m, k,
                       a["d_proof"], a["d_proof_lens"], a["d_counts"], a["d_leaves_out"], a["d_n_bad"])

    def call_v(a, stride=P):
        return verify(tag, a["d_tree_ids"], a["d_counts"], a["d_first"], a["d_leaf_offsets"], m, max_leaves, a["d_leaves_out"], k, a["d_proof"], stride,
                      a["d_proof_lens"], a["d_roots"], n_trees, a["d_ok"], a["d_roots_out"], a["d_n_hashed"], a["d_n_bad"])
    e_sym, v_sym = "p252_merkle%d_forest_ragged_range_proofs_device_into" % arity, "p252_merkle%d_forest_range_verify_device_into" % arity
    call_e(args)
    call_v(args)
    assert recorder.calls == [e_sym, v_sym]  # the control: the library is reached, once each, under this arity's symbols
    del recorder.calls[:]
    e_names = ("d_leaves", "d_offsets", "d_levels", "d_tree_ids", "d_first", "d_leaf_offsets", "d_proof", "d_proof_lens", "d_counts", "d_leaves_out", "d_n_bad")
    v_names = ("d_tree_ids", "d_counts", "d_first", "d_leaf_offsets", "d_leaves_out", "d_proof", "d_proof_lens", "d_roots", "d_ok", "d_roots_out", "d_n_hashed", "d_n_bad")
    for call, names, rename in ((call_e, e_names, {"d_counts": "d_counts_out"}), (call_v, v_names, {"d_leaves_out": "d_leaves_in"})):
        for where, bad in with_cpu_tensor({n: args[n] for n in names}):
            with pytest.raises(ValueError, match=rename.get(where, where) + " is on cpu"):
                call(dict(args, **bad))
    for name, short in (("d_offsets", dev(n=n_trees)), ("d_tree_ids", dev(i32, n=m - 1)), ("d_first", dev(n=m - 1)), ("d_leaf_offsets", dev(n=m)),
                        ("d_proof", dev(n=m * P * 4 - 1)), ("d_proof_lens", dev(i32, n=m - 1)), ("d_leaves_out", dev(n=k * 4 - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call_e(dict(args, **{name: short}))
    for name, short in (("d_counts", dev(n=m - 1)), ("d_roots", dev(n=n_trees * 4 - 1)), ("d_ok", dev(u8, n=m - 1)), ("d_roots_out", dev(n=m * 4 - 1)),
                        ("d_proof", dev(n=m * P * 4 - 1))):
        with pytest.raises(ValueError, match=name + " holds"):
            call_v(dict(args, **{name: short}))
    for name in ("d_first", "d_leaf_offsets", "d_counts", "d_n_hashed"):
        with pytest.raises(ValueError, match="needs 8-byte elements"):
            call_v(dict(args, **{name: dev(i32, n=64)}))
    for name in ("d_tree_ids", "d_proof_lens", "d_n_bad"):
        with pytest.raises(ValueError, match=name + " needs 4-byte elements"):
            call_v(dict(args, **{name: dev(n=64)}))
    with pytest.raises(ValueError, match="d_proof must be a torch tensor"):
        call_e(dict(args, d_proof=None))
    assert recorder.calls == []
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
    call_e(args)
    call_e(dict(args, d_levels=None, d_proof=None, d_leaves_out=None, d_n_bad=None), max_leaves=1)
    call_v(args)
    call_v(dict(args, d_proof=None, d_roots_out=None, d_n_hashed=None, d_n_bad=None), stride=0)
    a, b, c, d = seen
    ptr = lambda name: args[name].data_ptr()  # noqa: E731
    assert a[1:] == (ptr("d_leaves"), 120, ptr("d_offsets"), n_trees, max_leaves, ptr("d_levels"), ptr("d_tree_ids"), ptr("d_first"), ptr("d_leaf_offsets"),
                     m, k, ptr("d_leaves_out"), ptr("d_proof"), ptr("d_proof_lens"), ptr("d_counts"), ptr("d_n_bad"), 0)
    assert b[5:7] == (1, None) and b[12:14] == (None, None) and b[16] is None
    assert c[2:] == (ptr("d_tree_ids"), ptr("d_counts"), ptr("d_first"), ptr("d_leaf_offsets"), m, max_leaves, ptr("d_leaves_out"), k, ptr("d_proof"), P,
                     ptr("d_proof_lens"), ptr("d_roots"), n_trees, ptr("d_ok"), ptr("d_roots_out"), ptr("d_n_hashed"), ptr("d_n_bad"), 0)
    assert d[10:12] == (None, 0) and d[16:19] == (None, None, None)


def test_the_model_imports_nothing_of_the_library():
    src = open(os.path.join(ROOT, "testsupport", "forestrange.py")).read()
    imports = re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", src, re.M)
    assert set(imports) <= {"numpy", "."} and "poseidon252_amd" not in src and "torch" not in "".join(imports)


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_range_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_range_bench")
