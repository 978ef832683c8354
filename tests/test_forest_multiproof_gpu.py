"""The shared proof across a ragged forest (p252_merkle{4,2}_forest_ragged_multiproof_device_into / _verify_device;
csrc/forest_multiproof.hip) on the GPU: the proof offsets, the proof's bytes, the leaves, the recomputed roots and the digest count
against the model (testsupport/multiproofmodel.py: a composition of the single-tree model), every tree's part against the
existing single-tree call, the roots against the oracle; forests whose tree borders fall inside and on the edges of the scan tiles and
that reach both digest kernels; rejection per tree, bad pairs, a short proof buffer, edge values, streams, p252_trim, the conveniences,
the C++ mirror, and the time against the per-tree loop of the single-tree calls."""
import time

import numpy as np
import pytest

import edgecases as E
from helpers.forest import SENTINEL, _np, _single_extract, _single_verify, _tag, _torch
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport.multiproofmodel import forest_multiproof_counts, forest_multiproof_extract, forest_pairs_by_tree
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

SENT64 = np.uint64(SENTINEL & (2 ** 64 - 1))
SIZES = [5, 300, 1, 17, 66, 0, 64, 1000, 2, 16]  # (arity 4: 64 and 16 are complete trees; 0 is an empty tree, bad only if named)
_FORESTS = {}


class Forest:
    """a forest built once with its levels: host copies (leaves, compact tree-major levels, roots) and the device tensors"""

    def __init__(self, ctx, arity, sizes, leaves):
        import torch
        self.arity, self.sizes, self.T, self.top = arity, np.asarray(sizes, dtype=np.int64), len(sizes), int(max(sizes))
        self.off = TS.offsets(sizes, dtype=np.int64)
        self.n, self.leaves = int(self.off[-1]), leaves
        self.lo = TS.offsets(TS.levels_len(sizes, arity), dtype=np.int64)
        self.d, self.d_off = _torch(leaves), _torch(self.off.astype(np.uint64))
        self.d_lv = torch.zeros((max(TS.levels_bound(self.n, self.T, self.top, arity), 1), 4), dtype=torch.int64, device=self.d.device)
        self.d_roots = torch.zeros((self.T, 4), dtype=torch.int64, device=self.d.device)
        ctx.merkle_forest_ragged_device(_tag(arity), self.d, self.d_off, self.T, self.top, self.d_roots, d_levels=self.d_lv, arity=arity)
        torch.cuda.synchronize()
        self.levels, self.roots = _np(self.d_lv)[:self.lo[-1]], _np(self.d_roots)

    def tree(self, t):
        """tree t's block as the single-tree calls take it: (n, leaves, levels) device views"""
        n = int(self.sizes[t])
        return n, self.d[self.off[t]:self.off[t + 1]], self.d_lv[self.lo[t]:max(self.lo[t + 1], self.lo[t] + 1)]


def _leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60)"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(n, 4), dtype=np.uint64)


def _forest(ctx, arity, name="ten"):
    if (arity, name) not in _FORESTS:
        if name == "ten":
            sizes = SIZES
        elif name == "many":  # tree borders inside and on the edges of 256-element tiles
            sizes = np.random.default_rng(77).integers(16, 41, size=3000).tolist()
        else:  # "one": a single large tree alone in a forest
            sizes = [4 ** 7 + 5]
        _FORESTS[(arity, name)] = Forest(ctx, arity, sizes, _leaves(int(sum(sizes)), 31 * arity + len(sizes)))
    return _FORESTS[(arity, name)]


def _bound(ctx, f, k):
    fn = ctx.merkle4_forest_ragged_multiproof_bound if f.arity == 4 else ctx.merkle2_forest_ragged_multiproof_bound
    return fn(f.n, f.T, f.top, k)


def _extract(ctx, f, tid, lid, cap=None, pad=0):
    """one extraction -> (leaves_out (k + pad, 4), the whole proof buffer (bound + pad, 4), proof_offsets (T + 1,) uint64, n_bad); the
    call sees the first k rows / the first `cap` (default: bound) rows only, the rest holds the sentinel"""
    import torch
    k, dev = len(tid), f.d.device
    bound = _bound(ctx, f, k)
    cap = bound if cap is None else cap
    out = torch.full((k + pad, 4), SENTINEL, dtype=torch.int64, device=dev)
    proof = torch.full((bound + pad, 4), SENTINEL, dtype=torch.int64, device=dev)
    po = torch.full((f.T + 1,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call = ctx.merkle4_forest_ragged_multiproof_device if f.arity == 4 else ctx.merkle2_forest_ragged_multiproof_device
    call(f.d, f.d_off, f.T, f.top, f.d_lv, _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64)), k, out[:k],
         proof[:cap] if cap else None, po, d_n_bad=bad)
    ctx.sync()
    return _np(out), _np(proof), _np(po), int(bad)


def _verify(ctx, f, tid, lid, leaves, proof, proof_len, po, roots=None):
    """one verification of numpy inputs -> (ok (T,), roots_out (T, 4) with the sentinel where untouched, n_hashed, n_bad)"""
    import torch
    dev = f.d.device
    ok = torch.full((f.T,), 7, dtype=torch.uint8, device=dev)
    roots_out = torch.full((f.T, 4), SENTINEL, dtype=torch.int64, device=dev)
    hashed = torch.full((1,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    d_proof = _torch(np.ascontiguousarray(proof, dtype=np.uint64)) if len(proof) else None
    call = ctx.merkle4_forest_ragged_multiproof_verify_device if f.arity == 4 else ctx.merkle2_forest_ragged_multiproof_verify_device
    call(_tag(f.arity), f.d_off, f.n, f.T, f.top, _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64)),
         _torch(np.ascontiguousarray(leaves, dtype=np.uint64)), len(tid), d_proof, proof_len, _torch(np.asarray(po, np.uint64)),
         f.d_roots if roots is None else _torch(np.ascontiguousarray(roots, dtype=np.uint64)), ok, d_roots_out=roots_out, d_n_hashed=hashed, d_n_bad=bad)
    ctx.sync()
    return _np(ok), _np(roots_out), int(hashed), int(bad)


def _untouched(roots_out, t):
    return bool((roots_out[t] == SENT64).all())


def _has(f, tid):
    has = np.zeros(f.T, dtype=bool)
    has[np.asarray(tid, dtype=np.int64)] = True
    return has


def _round_trip(ctx, f, tid, lid):
    """extract + verify of ascending pairs, everything compared with the model and the build's roots"""
    tid, lid = np.asarray(tid, dtype=np.int64), np.asarray(lid, dtype=np.int64)
    want_out, want_proof, want_po = forest_multiproof_extract(f.leaves, f.off, f.levels, tid, lid, f.arity)
    want_po2, want_hashed = forest_multiproof_counts(f.sizes, tid, lid, f.arity)
    assert np.array_equal(want_po, want_po2) and int(want_po[-1]) <= _bound(ctx, f, len(tid))
    out, proof, po, bad = _extract(ctx, f, tid, lid)
    print("arity %d, %d trees, k %d: proof %d scalars (model %d), bad %d" % (f.arity, f.T, len(tid), int(po[-1]), int(want_po[-1]), bad))
    assert bad == 0 and np.array_equal(po, want_po)
    plen = int(po[-1])
    assert np.array_equal(proof[:plen], want_proof) and np.array_equal(out, want_out)
    ok, roots_out, hashed, bad = _verify(ctx, f, tid, lid, out, proof[:plen], plen, po)
    has = _has(f, tid)
    print("  verify: ok on %d trees (%d have pairs), n_hashed %d (model %d), bad %d" % (int(ok.sum()), int(has.sum()), hashed, want_hashed, bad))
    assert np.array_equal(ok.astype(bool), has) and (hashed, bad) == (want_hashed, 0)
    assert np.array_equal(roots_out[has], f.roots[has]) and all(_untouched(roots_out, t) for t in np.nonzero(~has)[0])
    return out, proof[:plen], po


def _pair_sets(sizes):
    live = [t for t, n in enumerate(sizes) if n > 0]
    sets = {"first": [(t, 0) for t in live], "last": [(t, sizes[t] - 1) for t in live],
            "every other": [(t, i) for t in live for i in range(0, sizes[t], 2)], "all": [(t, i) for t in live for i in range(sizes[t])],
            "two trees": [(1, i) for i in (0, 7, 8, 299)] + [(7, i) for i in range(500, 520)], "one pair": [(4, 65)]}
    return {k: (np.array([p[0] for p in v]), np.array([p[1] for p in v])) for k, v in sets.items()}


# ---- 1. against the single-tree call and the model ----
@pytest.mark.parametrize("arity", [4, 2])
def test_proof_and_verification_match_the_model_and_the_single_tree_call(gpu_ctx, oracle_mod, arity):
    f = _forest(gpu_ctx, arity)
    for t, n in enumerate(SIZES):  # the build's roots are the oracle's (a one-leaf tree: its leaf, here below p)
        if n:
            assert np.array_equal(f.roots[t], E.oracle_tree(_tag(arity), f.leaves[f.off[t]:f.off[t + 1]], arity)[0]), (arity, t)
    for name, (tid, lid) in _pair_sets(SIZES).items():
        out, proof, po = _round_trip(gpu_ctx, f, tid, lid)
        po = po.astype(np.int64)
        for t, pos in forest_pairs_by_tree(f.T, tid, lid).items():  # each segment is what the existing call returns for that tree block
            n, d, d_lv = f.tree(t)
            s_out, s_proof, s_len, s_bad = _single_extract(gpu_ctx, arity, n, d, d_lv, pos)
            assert (s_len, s_bad) == (po[t + 1] - po[t], 0), (name, t)
            assert np.array_equal(s_proof[:s_len], proof[po[t]:po[t + 1]]) and np.array_equal(s_out, out[tid == t]), (name, t)
        if name in ("every other", "two trees"):  # one tree's segment, cut out, under the existing single-tree verify
            t = 7
            ok, root_out, _, _ = _single_verify(gpu_ctx, arity, SIZES[t], lid[tid == t], out[tid == t], proof[po[t]:po[t + 1]], po[t + 1] - po[t],
                                                f.roots[t])
            assert ok == 1 and np.array_equal(root_out, f.roots[t]), name


# ---- 2. scan tiles and both digest kernels ----
def _many_pairs(f, per_tree, seed=9):
    rng = np.random.default_rng(seed)
    tid, lid = [], []
    for t, n in enumerate(f.sizes):
        pos = np.sort(rng.choice(int(n), min(per_tree, int(n)), replace=False))
        tid.append(np.full(pos.size, t))
        lid.append(pos)
    return np.concatenate(tid), np.concatenate(lid)


def test_tree_borders_inside_scan_tiles_and_the_one_lane_digest(gpu_ctx):
    f = _forest(gpu_ctx, 4, "many")
    tid, lid = _many_pairs(f, 12)
    level1 = sum(np.unique(pos // 4).size for pos in forest_pairs_by_tree(f.T, tid, lid).values())
    assert level1 > 8192 and len(tid) > 256 * 100  # past the lane-group kernel's batch; many tiles, their borders anywhere in a tree
    _round_trip(gpu_ctx, f, tid, lid)
    f2 = _forest(gpu_ctx, 2, "many")
    _round_trip(gpu_ctx, f2, tid, lid)


def test_forty_pairs_in_three_thousand_trees_run_on_the_lane_group_digest(gpu_ctx):
    f = _forest(gpu_ctx, 4, "many")
    trees = np.sort(np.random.default_rng(4).choice(f.T, 40, replace=False))
    _round_trip(gpu_ctx, f, trees, (f.sizes[trees] // 2))


@pytest.mark.parametrize("arity", [4, 2])
def test_one_large_tree_alone_in_a_forest_equals_the_single_tree_call(gpu_ctx, arity):
    f = _forest(gpu_ctx, arity, "one")
    lid = np.arange(3, 3003)
    out, proof, po = _round_trip(gpu_ctx, f, np.zeros(lid.size, dtype=np.int64), lid)
    n, d, d_lv = f.tree(0)
    s_out, s_proof, s_len, s_bad = _single_extract(gpu_ctx, arity, n, d, d_lv, lid)
    assert (s_len, s_bad) == (int(po[1]), 0) and np.array_equal(s_proof[:s_len], proof) and np.array_equal(s_out, out)


# ---- 3. rejection is per tree ----
@pytest.mark.parametrize("arity", [4, 2])
def test_rejection_is_per_tree(gpu_ctx, arity):
    f = _forest(gpu_ctx, arity)
    tid, lid = _pair_sets(SIZES)["every other"]
    out, proof, po = _round_trip(gpu_ctx, f, tid, lid)
    plen, has = int(po[-1]), _has(f, tid)
    po_i = po.astype(np.int64)

    def only(t, ok):
        want = has.copy()
        want[t] = False
        return np.array_equal(ok.astype(bool), want)
    changed = proof.copy()
    changed[(po_i[1] + po_i[2]) // 2, 1] ^= np.uint64(1)  # one proof scalar of tree 1's segment
    ok, roots_out, _, _ = _verify(gpu_ctx, f, tid, lid, out, changed, plen, po)
    assert only(1, ok) and not np.array_equal(roots_out[1], f.roots[1])
    leaves = out.copy()
    leaves[np.nonzero(tid == 7)[0][3], 0] ^= np.uint64(1)  # one leaf of tree 7
    ok, _, _, _ = _verify(gpu_ctx, f, tid, lid, leaves, proof, plen, po)
    assert only(7, ok)
    roots = f.roots.copy()
    roots[3, 2] ^= np.uint64(1)  # a wrong expected root
    ok, roots_out, _, _ = _verify(gpu_ctx, f, tid, lid, out, proof, plen, po, roots=roots)
    assert only(3, ok) and np.array_equal(roots_out[3], f.roots[3])
    # lying offsets: tree 4's end is also the start of tree 5, which nobody asks about
    t = 4
    assert po_i[t + 1] > po_i[t] and SIZES[t + 1] == 0
    for what, value in (("one less", po_i[t + 1] - 1), ("one more", po_i[t + 1] + 1), ("past proof_len", plen + 5), ("decreasing", po_i[t] - 1)):
        lie = po.copy()
        lie[t + 1] = value
        ok, roots_out, _, _ = _verify(gpu_ctx, f, tid, lid, out, proof, plen, lie)
        assert only(t, ok) and _untouched(roots_out, t), what
        assert all(np.array_equal(roots_out[u], f.roots[u]) for u in np.nonzero(has)[0] if u != t), what
    ok, roots_out, _, _ = _verify(gpu_ctx, f, tid, lid, out, proof[:plen - 1], plen - 1, po)  # one scalar short: the last tree with pairs only
    last = int(np.nonzero(has)[0][-1])
    assert po_i[last + 1] == plen and only(last, ok) and _untouched(roots_out, last)


# ---- 4. bad pairs ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_bad_pair_spoils_the_batch_and_is_counted_once(gpu_ctx, arity):
    f = _forest(gpu_ctx, arity)
    good_t, good_l = np.array([0, 1, 1, 3, 7, 7, 9]), np.array([2, 5, 6, 16, 0, 999, 15])
    cases = {"unsorted across trees": (np.array([0, 3, 1, 7]), np.array([2, 5, 6, 0]), 1),
             "unsorted within a tree": (np.array([1, 1, 1, 7]), np.array([5, 9, 8, 0]), 1),
             "a duplicate": (np.array([1, 1, 1, 7]), np.array([5, 8, 8, 0]), 1),
             "leaf id = n_t": (np.array([0, 3, 7]), np.array([2, 17, 0]), 1),
             "leaf id = 2^40": (np.array([0, 3, 7]), np.array([2, 1 << 40, 0]), 1),
             "tree id = n_trees": (np.array([0, 3, len(SIZES)]), np.array([2, 5, 0]), 1),
             "tree id = 0xFFFFFFFF": (np.array([0, 3, 0xFFFFFFFF]), np.array([2, 5, 0]), 1),
             "a pair in the empty tree": (np.array([0, 5, 7]), np.array([2, 0, 0]), 1),
             "two of them": (np.array([0, 3, 3, 7, 7]), np.array([2, 17, 18, 5, 5]), 3)}
    for name, (tid, lid, n_bad) in cases.items():
        out, proof, po, bad = _extract(gpu_ctx, f, tid, lid)
        assert bad == n_bad and not po.any(), (name, bad, po)
        ok, roots_out, hashed, bad = _verify(gpu_ctx, f, tid, lid, np.zeros((len(tid), 4), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64), 4,
                                             np.zeros(f.T + 1, dtype=np.uint64))
        assert bad == n_bad and hashed == 0 and not ok.any() and (roots_out == SENT64).all(), (name, bad, hashed, ok)
    _round_trip(gpu_ctx, f, good_t, good_l)  # afterwards a good call on the same context works


# ---- 5. a short proof buffer ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_short_proof_buffer_reports_the_need_and_writes_no_further(gpu_ctx, arity):
    f = _forest(gpu_ctx, arity)
    tid, lid = _pair_sets(SIZES)["first"]
    _, want, want_po = forest_multiproof_extract(f.leaves, f.off, f.levels, tid, lid, arity)
    need = int(want_po[-1])
    assert need > 8
    for cap in (0, 1, need // 2, need - 1, need):
        out, proof, po, bad = _extract(gpu_ctx, f, tid, lid, cap=cap, pad=3)
        assert bad == 0 and np.array_equal(po, want_po), cap  # the offsets always report the need
        assert np.array_equal(proof[:cap], want[:cap]) and (proof[cap:] == SENT64).all(), cap
        assert (out[len(tid):] == SENT64).all() and np.array_equal(out[:len(tid)], f.leaves[f.off[tid] + lid])


# ---- 6. edge values ----
@pytest.mark.parametrize("arity", [4, 2])
def test_edge_values_are_copied_as_bytes_and_hashed_mod_p(gpu_ctx, oracle_mod, arity):
    sizes = [1, 21, 1, 70, 6]
    raw, red = E.edge_scalars(0xF0 + arity, sum(sizes))
    fixed = [0, 1, E.P - 1, E.P, (1 << 256) - 1, E.PATTERNS[12]]  # 0, 1, p - 1, p, 2^256 - 1 and the saturated limbs, in tree 3
    for i, v in enumerate(fixed):
        raw[23 + 5 * i], red[23 + 5 * i] = E.limbs(v), E.limbs(v % E.P)
    raw[0], red[0] = E.limbs(E.P + 1), E.limbs(1)  # a one-leaf tree holding p + 1
    f = Forest(gpu_ctx, arity, sizes, raw)
    off = f.off
    for t, n in enumerate(sizes):  # the build's roots are the oracle's on the values mod p
        assert np.array_equal(f.roots[t], E.oracle_tree(_tag(arity), red[off[t]:off[t + 1]], arity)[0]), t
    assert np.array_equal(f.roots[0], E.limbs(1))
    tid = np.array([0] + [1] * 5 + [2] + [3] * 12 + [4] * 2)
    lid = np.array([0, 0, 3, 4, 11, 20, 0] + list(range(0, 60, 5)) + [1, 5])
    out, proof, po, bad = _extract(gpu_ctx, f, tid, lid)
    want_out, want_proof, want_po = forest_multiproof_extract(raw, off, f.levels, tid, lid, arity)
    assert bad == 0 and np.array_equal(po, want_po) and np.array_equal(out, want_out) and np.array_equal(proof[:int(po[-1])], want_proof)
    assert np.array_equal(out, raw[off[tid] + lid])  # extraction copies the bytes, reduced or not
    ok, roots_out, _, bad = _verify(gpu_ctx, f, tid, lid, out, proof[:int(po[-1])], int(po[-1]), po)
    assert bad == 0 and ok.all() and np.array_equal(roots_out, f.roots) and E.is_reduced(roots_out).all()


# ---- 7. streams and trim ----
def test_another_stream_and_a_trimmed_context_give_the_same_bytes(gpu_ctx):
    import torch
    f = _forest(gpu_ctx, 4)
    tid, lid = _pair_sets(SIZES)["every other"]
    first = _round_trip(gpu_ctx, f, tid, lid)
    with torch.cuda.stream(torch.cuda.Stream()):
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
        second = _round_trip(gpu_ctx, f, tid, lid)
    torch.cuda.synchronize()
    gpu_ctx.trim()
    assert gpu_ctx.scratch_residue() == 0
    third = _round_trip(gpu_ctx, f, tid, lid)
    for other in (second, third):
        assert all(np.array_equal(a, b) for a, b in zip(first, other))


# ---- 8. the conveniences and the C++ mirror ----
@pytest.mark.parametrize("arity", [4, 2])
def test_conveniences_sort_deduplicate_and_raise_on_an_outside_pair(gpu_ctx, arity):
    import poseidon252_amd as P
    f = _forest(gpu_ctx, arity)
    tid, lid = [7, 1, 7, 0, 1, 9], [500, 8, 3, 4, 8, 15]
    t, l, leaves, proof, po = P.forest_ragged_multiproof(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, tid, lid, arity=arity)
    assert t.cpu().tolist() == [0, 1, 7, 7, 9] and l.cpu().tolist() == [4, 8, 3, 500, 15]
    want_out, want_proof, want_po = forest_multiproof_extract(f.leaves, f.off, f.levels, t.cpu().numpy(), l.cpu().numpy(), arity)
    assert np.array_equal(_np(leaves), want_out) and np.array_equal(_np(proof), want_proof) and np.array_equal(_np(po), want_po)
    ok = P.forest_ragged_multiproof_verify(gpu_ctx, f.d_off, f.n, f.T, f.top, t, l, leaves, proof, po, f.d_roots, arity=arity)
    assert ok.tolist() == [u in (0, 1, 7, 9) for u in range(f.T)]
    for bad_t, bad_l in (([0, f.T], [0, 0]), ([0, 3], [0, 17]), ([5], [0]), ([0], [-1]), ([0], [1 << 40])):
        with pytest.raises(ValueError, match="outside the forest"):
            P.forest_ragged_multiproof(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, bad_t, bad_l, arity=arity)


def test_cpp_mirror_program_runs(gpu_ctx, oracle_mod, tmp_path):
    assert run_cpp_mirror(build_cpp_mirror("test_forest_multiproof_api", tmp_path), timeout=120).strip().endswith("ok")


# ---- 9. relative time, same run ----
def test_one_call_is_faster_than_the_loop_over_the_trees(gpu_ctx):
    """3,000 trees, about 12 pairs each: one forest extraction + one forest verification against 3,000 single-tree extractions and
    verifications over the same pairs (the only way to serve a forest before this call; launch-bound)."""
    import torch
    ctx = gpu_ctx
    f = _forest(ctx, 4, "many")
    tid, lid = _many_pairs(f, 12)
    k, dev = len(tid), f.d.device
    d_tid, d_lid = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64))
    out = torch.empty((k, 4), dtype=torch.int64, device=dev)
    proof = torch.empty((_bound(ctx, f, k), 4), dtype=torch.int64, device=dev)
    po, ok = torch.zeros(f.T + 1, dtype=torch.int64, device=dev), torch.zeros(f.T, dtype=torch.uint8, device=dev)
    ctx.merkle4_forest_ragged_multiproof_device(f.d, f.d_off, f.T, f.top, f.d_lv, d_tid, d_lid, k, out, proof, po)
    plen = int(po[-1])
    po_h = po.cpu().numpy()

    def forest():
        ctx.merkle4_forest_ragged_multiproof_device(f.d, f.d_off, f.T, f.top, f.d_lv, d_tid, d_lid, k, out, proof, po)
        ctx.merkle4_forest_ragged_multiproof_verify_device(_tag(4), f.d_off, f.n, f.T, f.top, d_tid, d_lid, out, k, proof, plen, po, f.d_roots, ok)
    jobs, at = [], 0
    for t, pos in sorted(forest_pairs_by_tree(f.T, tid, lid).items()):
        n, d, d_lv = f.tree(t)
        kt = pos.size
        jobs.append((n, d, d_lv, _torch(pos.astype(np.uint32)), kt, out[at:at + kt], proof[po_h[t]:max(po_h[t + 1], po_h[t] + 1)],
                     int(po_h[t + 1] - po_h[t]), f.d_roots[t]))
        at += kt
    plen1, ok1 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.uint8, device=dev)
    out1 = torch.empty((64, 4), dtype=torch.int64, device=dev)
    proof1 = torch.empty((256, 4), dtype=torch.int64, device=dev)
    oks = []

    def loop():
        del oks[:]
        for n, d, d_lv, idx, kt, lv_in, pf, length, root in jobs:
            ctx.merkle_multiproof_device(d, n, d_lv, idx, kt, out1[:kt], proof1, plen1, arity=4)
            ctx.merkle_multiproof_verify_device(_tag(4), n, idx, lv_in, kt, pf if length else None, length, root, ok1, arity=4)
    times = {forest: [], loop: []}
    for fn in (forest, loop):  # warm both
        fn()
    torch.cuda.synchronize()
    assert int(ok.sum()) == f.T and int(ok1) == 1
    for _ in range(3):  # alternate; the synchronise is inside the timed window
        for fn in (forest, loop):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[fn].append(time.perf_counter() - t0)
    one, many = float(np.median(times[forest])), float(np.median(times[loop]))
    print("forest extraction + verification of %d pairs in %d trees: %.3f ms; the loop of single-tree calls: %.1f ms; ratio %.1f"
          % (k, f.T, one * 1e3, many * 1e3, many / one))
    assert one < many
