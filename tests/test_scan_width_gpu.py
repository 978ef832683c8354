"""Every two-level scan of the ragged calls driven past one block of tiles on the GPU (the shapes of tests/scanwidth.py, whose
conditions tests/test_scan_width_cpu.py asserts), byte for byte against expectations that share none of those scans: the forest by size
class through hash_batch, the numpy models of testsupport/, and the oracle on the trees at the trip borders.

No difference from the models or the oracle was found at these widths.  The dense single-tree proofs hold 5,243 scalars only (the
dropped leaves), so their rejected node is the proof's last one; the sparse proofs (112,842 and 90,393 scalars) have theirs beyond
offset 65,536."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edgecases as E
import scanwidth as S
from testsupport.forestupdate import dirty_nodes
from testsupport.device import tree_device
from testsupport.multiproofmodel import multiproof_counts, multiproof_extract
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
_WIDE, _FM = {}, {}


def _gpu_digest(ctx, arity):
    tag = E._mtag(arity)
    return lambda ch: ctx.hash_batch(tag, np.ascontiguousarray(ch), arity, 1).reshape(-1, 4)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first at %d, last at %d" % (what, rows.size, got.shape[0], int(rows[0]), int(rows[-1])))


class _Wide:
    """the wide forest built once per arity (with levels, into sentinel buffers) and its expectation"""

    def __init__(self, ctx, arity):
        f = self.f = S.wide_forest(arity)
        self.d, self.d_off, self.d_roots, self.d_lv, self.bad = S.run_build(ctx, arity, f.flat, f.off, f.max_leaves)
        self.roots, self.levels, self.lo = S.expected_forest(f.sizes, f.off, f.flat, arity, _gpu_digest(ctx, arity))
        self.used = int(self.lo[-1])


def _wide(ctx, arity):
    if arity not in _WIDE:
        _WIDE[arity] = _Wide(ctx, arity)
    return _WIDE[arity]


def _oracle_check(arity, sizes, off, flat, lo, roots, levels, ids, what):
    built = S.oracle_trees(arity, sizes, off, flat, ids)
    for t in ids:
        assert np.array_equal(roots[t], built[t][0]), "%s: the root of tree %d (%d leaves) is not the oracle's" % (what, t, sizes[t])
        assert np.array_equal(levels[lo[t]:lo[t + 1]], built[t][1]), "%s: the levels of tree %d (%d leaves) are not the oracle's" % (what, t, sizes[t])


# ---------------------------------------------------------------------------------------------- the wide forest
@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_forest_build(gpu_ctx, oracle_mod, arity):
    w = _wide(gpu_ctx, arity)
    f = w.f
    assert w.bad == 0
    roots, levels = E._host(w.d_roots), E._host(w.d_lv)
    _same(roots, w.roots, "roots")
    _same(levels[:w.used], w.levels, "levels")
    assert (levels[w.used:] == S.SENT64).all(), "levels written at or past the used length"
    _, _, r_only, _, bad = S.run_build(gpu_ctx, arity, f.flat, f.off, f.max_leaves, want_levels=False, d=w.d)
    assert bad == 0
    _same(E._host(r_only), w.roots, "roots of the roots-only build")
    _oracle_check(arity, f.sizes, f.off, f.flat, w.lo, roots, levels, f.oracle_ids, "build")
    assert np.array_equal(roots[f.unreduced], E.reduce_mod_p(f.flat[f.off[f.unreduced]]))  # a one-leaf tree's root: its leaf mod p


def _pairs(f, k, seed, distinct_trees):
    """k (tree, leaf) pairs that include the border trees and the unreduced one-leaf trees, ascending in the tree"""
    rng = np.random.default_rng(seed)
    T = f.sizes.size
    must = np.array(sorted(set(S.trip_borders(T)) | set(f.unreduced) | {0, T - 1}), dtype=np.int64)
    more = rng.choice(T, k, replace=False)
    tid = np.sort(np.concatenate([must, np.setdiff1d(more, must)[:k - must.size]]))
    assert tid.size == k and (not distinct_trees or np.unique(tid).size == k)
    lid = (rng.random(k) * f.sizes[tid]).astype(np.int64)
    return tid, lid


@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_forest_openings(gpu_ctx, arity):
    import torch
    w = _wide(gpu_ctx, arity)
    f, ctx, k = w.f, gpu_ctx, 5000
    T, tag = f.sizes.size, E._mtag(arity)
    tid, lid = _pairs(f, k, 0x09E + arity, False)
    d_tid, d_lid = E._dev(tid.astype(np.uint32)), E._dev(lid.astype(np.uint64))
    bad = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    o_l, o_s, o_p, o_d, D = ctx.merkle_forest_ragged_openings_device(w.d, w.d_off, T, f.max_leaves, w.d_lv, d_tid, d_lid, k, d_n_bad=bad[:1], arity=arity)
    back = torch.full((k, 4), S.SENTINEL, dtype=torch.int64, device="cuda:0")
    ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda:0")
    ctx.merkle_path_ragged_device(tag, o_l, o_s, o_p, o_d, D, back, k, d_n_bad=bad[1:], arity=arity)
    ctx.merkle_forest_ragged_verify_device(tag, o_l, o_s, o_p, o_d, D, d_tid, w.d_roots, T, ok, k, arity=arity)
    torch.cuda.synchronize()
    assert D == TS.depth(f.max_leaves, arity) and E._host(bad).tolist() == [0, 0]
    sib, pos, depths = S.expected_siblings(f.sizes, f.off, f.flat, w.lo, w.levels, tid, lid, arity, D)
    _same(E._host(o_l), f.flat[f.off[tid] + lid], "the opened leaves")
    _same(E._host(o_d).astype(np.int64), depths, "depths")
    _same(E._host(o_p).reshape(k, D), pos, "positions")
    _same(E._host(o_s).reshape(k, D, arity - 1, 4), sib, "siblings")
    _same(E._host(back), w.roots[tid], "path_ragged's roots")
    assert (E._host(ok) == 1).all(), "opening %d does not verify" % int(np.argmin(E._host(ok) == 1))


@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_forest_update(gpu_ctx, oracle_mod, arity):
    import torch
    w = _wide(gpu_ctx, arity)
    f, ctx, k = w.f, gpu_ctx, 5000
    T = f.sizes.size
    tid, lid = _pairs(f, k, 0x0BD + arity, True)
    new = S.leaves(k, 0xBD0 + arity)
    order = np.random.default_rng(arity).permutation(k)  # (the call takes the pairs in any order)
    d, lv, roots = w.d.clone(), w.d_lv.clone(), w.d_roots.clone()
    bad, hashed = torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ctx.merkle_forest_ragged_update_device(E._mtag(arity), d, w.d_off, T, f.max_leaves, lv, E._dev(tid[order].astype(np.uint32)),
                                           E._dev(lid[order].astype(np.uint64)), E._dev(new[order]), k, d_roots=roots, d_n_bad=bad,
                                           d_n_hashed=hashed, arity=arity)
    torch.cuda.synchronize()
    flat = f.flat.copy()
    flat[f.off[tid] + lid] = new
    want_roots, want_levels, lo = S.expected_forest(f.sizes, f.off, flat, arity, _gpu_digest(ctx, arity))
    assert int(bad) == 0 and int(hashed) == dirty_nodes(f.sizes, tid, lid, arity)
    _same(E._host(d), flat, "leaves")
    got_lv, got_roots = E._host(lv), E._host(roots)
    _same(got_lv[:w.used], want_levels, "levels")
    assert (got_lv[w.used:] == S.SENT64).all()
    _same(got_roots, want_roots, "roots")
    ids = sorted(set(S.trip_borders(T)) | {0, T - 1} | set(f.unreduced))
    _oracle_check(arity, f.sizes, f.off, flat, lo, got_roots, got_lv, ids, "update")


def _against_fresh_build(ctx, arity, out, flat, off, max_leaves, model, what, rng):
    """an append's / resize's outputs against the model's forest and a fresh build of it; the oracle on the border trees of the new numbering"""
    o_leaves, o_off, o_lv, o_roots, bad, hashed = out
    sizes = np.diff(off)
    n_new, want_hashed, want_bad = model
    assert np.array_equal(sizes, n_new)
    _same(E._host(o_off).astype(np.int64), off, what + ": offsets")
    got_leaves = E._host(o_leaves)
    _same(got_leaves[:off[-1]], flat, what + ": leaves")
    assert (got_leaves[off[-1]:] == S.SENT64).all()
    assert (bad, hashed) == (want_bad, want_hashed), "%s: n_bad %d (model %d), n_hashed %d (model %d)" % (what, bad, want_bad, hashed, want_hashed)
    _, _, f_roots, f_lv, f_bad = S.run_build(ctx, arity, flat, off, max_leaves)
    assert f_bad == want_bad
    used = int(TS.levels_len(sizes, arity).sum())
    got_lv, got_roots = E._host(o_lv), E._host(o_roots)
    _same(got_roots, E._host(f_roots), what + ": roots against a fresh build")
    _same(got_lv[:used], E._host(f_lv)[:used], what + ": levels against a fresh build")
    assert (got_lv[used:] == S.SENT64).all()
    T = sizes.size
    ids = [t for t in S.oracle_share(T, [T - 2, T - 3], rng, 100) if sizes[t]]
    _oracle_check(arity, sizes, off, flat, TS.block_starts(sizes, arity), got_roots, got_lv, ids, what)
    assert not got_roots[sizes == 0].any()


@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_forest_append_and_resize(gpu_ctx, oracle_mod, arity):
    w = _wide(gpu_ctx, arity)
    f, ctx = w.f, gpu_ctx
    T = f.sizes.size
    rng = np.random.default_rng(arity)
    ap = S.wide_append(arity)
    out = S.run_resize(ctx, arity, (w.d, w.d_off, T, f.max_leaves, w.d_lv), ap, f.flat.shape[0])
    model = S.resize_counts(f.sizes, None, ap["m"], arity)
    flat2, off2 = S.resize_leaves(f.off, f.flat, np.concatenate([f.sizes, np.zeros(ap["T_new"] - T, dtype=np.int64)]), ap["add_off"], ap["add"])
    _against_fresh_build(ctx, arity, out, flat2, off2, ap["max_new"], model, "append", rng)
    # the resize, on what the append wrote
    rs = S.wide_resize(arity, model[0])
    out3 = S.run_resize(ctx, arity, (out[0], out[1], ap["T_new"], ap["max_new"], out[2]), rs, int(out[0].shape[0]))
    model3 = S.resize_counts(model[0], rs["keep"], rs["m"], arity)
    kept = np.minimum(rs["keep"], model[0][:rs["T_new"]].astype(np.uint64)).astype(np.int64)
    flat3, off3 = S.resize_leaves(off2, flat2, kept, rs["add_off"], rs["add"])
    _against_fresh_build(ctx, arity, out3, flat3, off3, rs["max_new"], model3, "resize", rng)


# ---------------------------------------------------------------------------------------------- the single-tree multiproof
@pytest.mark.parametrize("case", ["dense", "sparse"])
@pytest.mark.parametrize("arity", S.ARITIES)
def test_single_tree_multiproof(gpu_ctx, oracle_mod, arity, case):
    import torch
    ctx, n, tag = gpu_ctx, S.single_n(arity), E._mtag(arity)
    pos = S.single_positions(arity, case)
    k = pos.size
    flat = S.leaves(n, 0x51 + arity)
    want_root, want_levels = S._cached(("single tree", arity), lambda: E.oracle_tree(tag, flat, arity))
    d = E._dev(flat)
    d_root = torch.empty(4, dtype=torch.int64, device="cuda:0")
    d_lv = torch.empty((want_levels.shape[0], 4), dtype=torch.int64, device="cuda:0")
    tree_device(ctx, arity, tag, d, n, d_root, d_lv)
    want = multiproof_extract(flat, want_levels, pos, arity)
    want_len, want_hashed = multiproof_counts(n, pos, arity)
    bound = ctx.merkle_multiproof_bound(n, k, arity)
    assert want.shape[0] == want_len <= bound
    out = torch.full((k, 4), S.SENTINEL, dtype=torch.int64, device="cuda:0")
    proof = torch.full((bound + 5, 4), S.SENTINEL, dtype=torch.int64, device="cuda:0")
    plen = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_idx = E._dev(pos.astype(np.uint32))
    ctx.merkle_multiproof_device(d, n, d_lv, d_idx, k, out, proof[:bound], plen, d_n_bad=bad, arity=arity)
    torch.cuda.synchronize()
    print("arity %d %s: k %d, proof_len %d (model %d), bad %d" % (arity, case, k, int(plen), want_len, int(bad)))
    assert np.array_equal(E._host(d_root), want_root) and np.array_equal(E._host(d_lv), want_levels)
    assert (int(plen), int(bad)) == (want_len, 0)
    got = E._host(proof)
    _same(got[:want_len], want, "proof")
    assert (got[want_len:] == S.SENT64).all()
    _same(E._host(out), flat[pos], "leaves_out")

    def verify(d_proof):
        ok = torch.full((1,), 7, dtype=torch.uint8, device="cuda:0")
        root_out = torch.full((4,), S.SENTINEL, dtype=torch.int64, device="cuda:0")
        hashed = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        ctx.merkle_multiproof_verify_device(tag, n, d_idx, out, k, d_proof, want_len, d_root, ok, d_root_out=root_out, d_n_hashed=hashed,
                                            d_n_bad=bad, arity=arity)
        torch.cuda.synchronize()
        return int(ok), E._host(root_out), int(hashed)
    ok, root_out, hashed = verify(proof[:want_len])
    assert (ok, hashed, int(bad)) == (1, want_hashed, 0) and np.array_equal(root_out, want_root)
    # one flipped limb in a proof node beyond the first chunk of the proof (a proof shorter than that: in its last node)
    at = S.LIST_CHUNK + (want_len - S.LIST_CHUNK) // 2 if want_len > S.LIST_CHUNK + 1 else want_len - 1
    assert case == "dense" or at > S.LIST_CHUNK
    flipped = proof[:want_len].clone()
    flipped[at, 2] = flipped[at, 2] ^ 4
    ok, root_out, _ = verify(flipped)
    assert ok == 0 and not np.array_equal(root_out, want_root)


# ---------------------------------------------------------------------------------------------- the forest multiproof
def _fm_expected(ctx, name, arity):
    """(flat, roots, levels, lo) of the case's forest: the wide forest's, or by size class through the oracle's digest"""
    c = S.FM_CASES[name](arity)
    if name == "wide":
        w = _wide(ctx, arity)
        return w.f.flat, w.roots, w.levels, w.lo
    key = ("fm expected", name.rstrip("012"), arity)
    flat = S.fm_leaves(name, arity)
    return (flat,) + S._cached(key, lambda: S.expected_forest(c.sizes, c.off, flat, arity, S.oracle_digest(arity)))


def _fm_run(ctx, name, arity):
    if (name, arity) not in _FM:
        c = S.FM_CASES[name](arity)
        w = _wide(ctx, arity) if name == "wide" else None
        built = (w.d, w.d_off, w.d_roots, w.d_lv, w.bad) if w else None
        _FM[(name, arity)] = S.run_forest_multiproof(ctx, c, S.fm_leaves(name, arity), built)
    return _FM[(name, arity)]


def _fm_check(c, r, want, roots, what):
    T = c.sizes.size
    has = np.zeros(T, dtype=bool)
    has[c.tid] = True
    length = int(want["po"][-1])
    assert r["bad"] == [0, 0] and r["build_bad"] == 0
    _same(r["po"], want["po"], what + ": proof_offsets")
    assert r["length"] == length <= r["bound"]
    _same(r["out"], want["out"], what + ": leaves_out")
    _same(r["proof"][:length], want["proof"], what + ": proof")
    assert (r["proof"][length:] == S.SENT64).all(), what + ": the proof buffer is written past the proof's length"
    _same(r["ok"].astype(bool), has, what + ": the verdicts")
    assert r["hashed"] == want["hashed"]
    _same(r["roots_out"][has], roots[has], what + ": the recomputed roots")
    assert (r["roots_out"][~has] == S.SENT64).all()
    after = has.copy()
    after[c.victim] = False
    _same(r["ok_changed"].astype(bool), after, what + ": the verdicts after one changed leaf of tree %d" % c.victim)


@pytest.mark.parametrize("name", sorted(S.FM_CASES))
@pytest.mark.parametrize("arity", S.ARITIES)
def test_forest_multiproof(gpu_ctx, oracle_mod, arity, name):
    import torch
    ctx = gpu_ctx
    c = S.FM_CASES[name](arity)
    flat, roots, levels, lo = _fm_expected(ctx, name, arity)
    assert flat.shape[0] == c.off[-1]
    r = _fm_run(ctx, name, arity)
    _same(r["roots"], roots, "the build's roots")
    want = S.forest_multiproof_fast(c.sizes, c.tid, c.lid, arity, c.off, flat, lo, levels)
    print("forest multiproof %s arity %d: %d pairs, proof %d scalars (model %d), lists %s" % (name, arity, c.tid.size, r["length"], int(want["po"][-1]),
                                                                                            want["counts"]))
    _fm_check(c, r, want, roots, "%s arity %d" % (name, arity))
    if c.big is not None:  # the big tree's part under the single-tree verify
        d, d_off, d_roots, lv, out, proof, po = r["d"]
        first = S.first_pair_index(c)
        lo_, hi_ = first[c.big], first[c.big + 1]
        p0, p1 = int(want["po"][c.big]), int(want["po"][c.big + 1])
        ok = torch.full((1,), 7, dtype=torch.uint8, device="cuda:0")
        root_out = torch.full((4,), S.SENTINEL, dtype=torch.int64, device="cuda:0")
        ctx.merkle_multiproof_verify_device(E._mtag(arity), int(c.sizes[c.big]), E._dev(c.lid[lo_:hi_].astype(np.uint32)), out[lo_:hi_], hi_ - lo_,
                                            proof[p0:p1], p1 - p0, d_roots[c.big], ok, d_root_out=root_out, arity=arity)
        torch.cuda.synchronize()
        assert int(ok) == 1 and np.array_equal(E._host(root_out), roots[c.big])


# ---------------------------------------------------------------------------------------------- the ragged hash
def _child(what, arity, tmp_path, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scanwidth.py"), "child", what, str(arity), str(tmp_path)],
                       env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_ragged_hash_long_messages(gpu_ctx, oracle_mod, tmp_path):
    import poseidon252_amd as P
    _child("ragged", 0, tmp_path, {"P252_RAGGED_SORT": "0"})
    unsorted = np.load(str(tmp_path / "ragged.npz"))
    for n in S.RAGGED_SIZES:
        flat, off, lens = S.ragged_batch(n)
        for out_len in (1, 5):
            want = S.ragged_oracle(flat, off, out_len)
            for truncated in (False, True):
                got = S.run_ragged(gpu_ctx, n, out_len, truncated)
                exp = P.truncate250(want) if truncated else want
                if not np.array_equal(got, exp):
                    rows = np.nonzero((got != exp).reshape(n, -1).any(axis=1))[0]
                    raise AssertionError("n %d out_len %d truncated %s: messages of lengths %s differ from the oracle" % (
                        n, out_len, truncated, sorted(set(lens[rows].tolist()))[:20]))
                assert np.array_equal(unsorted["%d_%d_%d" % (n, out_len, int(truncated))].view(np.uint64), got), (n, out_len, truncated)


# ---------------------------------------------------------------------------------------------- the one-lane digests
def test_one_lane_digests_in_a_child_process(gpu_ctx, tmp_path):
    """P252_COOP_MAX_NODES=0 is read once per process: the wide build (arity 4) and the wide forest multiproof (arity 2) in children"""
    env = {"P252_COOP_MAX_NODES": "0"}
    _child("build", 4, tmp_path, env)
    got = np.load(str(tmp_path / "build.npz"))
    w = _wide(gpu_ctx, 4)
    assert int(got["bad"]) == 0
    _same(got["roots"].view(np.uint64), w.roots, "roots of the one-lane build")
    assert np.array_equal(got["levels_sha256"], S._digest_of(w.levels)), "the levels of the one-lane build"
    _child("fm:wide", 2, tmp_path, env)
    got = np.load(str(tmp_path / "fm.npz"))
    r = _fm_run(gpu_ctx, "wide", 2)
    _same(got["po"].view(np.uint64), r["po"], "proof_offsets")
    _same(got["proof"].view(np.uint64), r["proof"][:r["length"]], "proof")
    assert np.array_equal(got["ok"], r["ok"]) and np.array_equal(got["ok_changed"], r["ok_changed"]) and int(got["hashed"]) == r["hashed"]
    _same(got["roots_out"].view(np.uint64), r["roots_out"], "the recomputed roots")
