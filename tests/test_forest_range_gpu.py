"""Whole runs of leaves of a ragged forest proved and checked in one call (p252_merkle{4,2}_forest_ragged_range_proofs_device_into /
p252_merkle{4,2}_forest_range_verify_device_into; csrc/forest_range.hip) on the GPU: the proofs, lengths, counts and leaves against the
numpy model (testsupport/forestrange.py) byte for byte, sampled rows against the single-tree shared proof of the same positions, the
verdicts, the recomputed roots and the digest count; one run past the 8-lane rule; whole trees; every kind of bad run on both calls;
every single change to a good batch; leaves at and above the modulus; two streams of one context."""
import numpy as np
import pytest

import edgecases as E
from helpers.forest import SENTINEL, _np, _single_extract, _tag, _torch
from testsupport import forestrange as FR
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

SENT64 = np.uint64(SENTINEL & (2 ** 64 - 1))
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257]
_FORESTS = {}


class Forest:
    """a forest built once with its levels: host copies (leaves, compact tree-major levels, roots) and the device tensors"""

    def __init__(self, ctx, arity, sizes, leaves):
        import torch
        self.arity, self.sizes, self.T, self.top = arity, np.asarray(sizes, dtype=np.int64), len(sizes), int(max(sizes))
        self.off = TS.offsets(sizes, dtype=np.int64)
        self.n, self.leaves = int(self.off[-1]), leaves
        self.lo = TS.block_starts(sizes, arity)
        self.d, self.d_off = _torch(leaves), _torch(self.off.astype(np.uint64))
        self.d_lv = torch.zeros((max(TS.levels_bound(self.n, self.T, self.top, arity), 1), 4), dtype=torch.int64, device=self.d.device)
        self.d_roots = torch.zeros((self.T, 4), dtype=torch.int64, device=self.d.device)
        ctx.merkle_forest_ragged_device(_tag(arity), self.d, self.d_off, self.T, self.top, self.d_roots, d_levels=self.d_lv, arity=arity)
        torch.cuda.synchronize()
        self.levels, self.roots = _np(self.d_lv)[:self.lo[-1]], _np(self.d_roots)
        self.stride = FR.range_stride(self.top, arity)


def _leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60)"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(n, 4), dtype=np.uint64)


def _forest(ctx, arity, name="twelve"):
    if (arity, name) not in _FORESTS:
        if name == "twelve":
            sizes = SIZES
        elif name == "bad tree":  # tree 2 is empty: bad for whoever names it
            sizes = [5, 17, 0, 65, 1, 16]
        else:  # "large": one tree of 4^9 (arity 2: 2^18) leaves and three small ones
            sizes = [4 ** 9 if arity == 4 else 2 ** 18, 17, 5, 64]
        _FORESTS[(arity, name)] = Forest(ctx, arity, sizes, _leaves(int(sum(sizes)), 53 * arity + len(sizes)))
    return _FORESTS[(arity, name)]


class Batch:
    """m runs as the two calls take them (numpy)"""

    def __init__(self, tid, first, lens=None, leaf_offsets=None):
        self.tid, self.first = np.asarray(tid, dtype=np.uint32), np.asarray(first, dtype=np.uint64)
        self.loff = TS.offsets(lens) if leaf_offsets is None else np.asarray(leaf_offsets, dtype=np.uint64)
        self.m = len(self.tid)


def _extract(ctx, f, B, k, with_leaves=True, n_trees=None):
    """one extraction -> (proof (m, P, 4), lens, counts, leaves_out (k, 4) — the sentinel where untouched —, n_bad); one row of
    sentinel scalars behind the proofs and the leaves must stay"""
    import torch
    dev = f.d.device
    proof = torch.full((B.m * f.stride + 1, 4), SENTINEL, dtype=torch.int64, device=dev)
    lens = torch.full((B.m,), 7, dtype=torch.int32, device=dev)
    counts = torch.full((B.m,), -1, dtype=torch.int64, device=dev)
    out = torch.full((k + 1, 4), SENTINEL, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call = ctx.merkle4_forest_ragged_range_proofs_device if f.arity == 4 else ctx.merkle2_forest_ragged_range_proofs_device
    call(f.d, f.d_off, f.T if n_trees is None else n_trees, f.top, f.d_lv, _torch(B.tid), _torch(B.first), _torch(B.loff), B.m, k, proof, lens, counts,
         d_leaves_out=out if with_leaves else None, d_n_bad=bad)
    ctx.sync()
    p, o = _np(proof), _np(out)
    assert (p[-1] == SENT64).all() and (o[-1] == SENT64).all()
    return p[:-1].reshape(B.m, f.stride, 4), _np(lens).view(np.uint32), _np(counts), o[:-1], int(bad)


def _verify(ctx, f, B, counts, leaves, proof, lens, roots=None, stride=None, max_leaves=None):
    """one verification of numpy inputs -> (ok (m,), roots_out (m, 4) with the sentinel where untouched, n_hashed, n_bad)"""
    import torch
    dev = f.d.device
    stride = f.stride if stride is None else stride
    ok = torch.full((B.m + 1,), 7, dtype=torch.uint8, device=dev)
    roots_out = torch.full((B.m + 1, 4), SENTINEL, dtype=torch.int64, device=dev)
    hashed = torch.full((1,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    d_roots = f.d_roots if roots is None else _torch(np.ascontiguousarray(roots, dtype=np.uint64))
    call = ctx.merkle4_forest_range_verify_device if f.arity == 4 else ctx.merkle2_forest_range_verify_device
    call(_tag(f.arity), _torch(B.tid), _torch(np.asarray(counts, dtype=np.uint64)), _torch(B.first), _torch(B.loff), B.m, f.top if max_leaves is None else max_leaves,
         _torch(np.ascontiguousarray(leaves, dtype=np.uint64)), len(leaves), _torch(np.ascontiguousarray(proof, dtype=np.uint64)), stride,
         _torch(np.asarray(lens, dtype=np.uint32)), d_roots, d_roots.shape[0], ok[:B.m], d_roots_out=roots_out[:B.m], d_n_hashed=hashed, d_n_bad=bad)
    ctx.sync()
    assert int(ok[-1]) == 7 and (_np(roots_out)[-1] == SENT64).all()
    return _np(ok)[:-1], _np(roots_out)[:-1], int(hashed), int(bad)


def _model_extract(f, B, k):
    return FR.range_extract(f.leaves, f.off, f.levels, B.tid, B.first, B.loff, k, f.top, f.arity, leaves_out=np.full((k, 4), SENT64))


def _model_verify(oracle_mod, f, B, counts, leaves, proof, lens, roots=None, max_leaves=None):
    digest = lambda kids: oracle_mod.hash_batch(_tag(f.arity), kids, f.arity, 1)  # noqa: E731
    return FR.range_verify(counts, B.tid, B.first, B.loff, len(leaves), f.top if max_leaves is None else max_leaves, leaves, proof, lens,
                           f.roots if roots is None else roots, f.arity, digest, E.reduce_mod_p)


def _round_trip(ctx, f, B):
    """extraction against the model byte for byte; verification: ok everywhere, the build's roots, the model's digest count"""
    k = int(B.loff[-1])
    want = _model_extract(f, B, k)
    proof, lens, counts, out, bad = _extract(ctx, f, B, k)
    print("arity %d: %d runs, %d leaves, proof scalars %d (model %d), bad %d" % (f.arity, B.m, k, int(lens.sum()), int(want[1].sum()), bad))
    assert bad == 0 == want[4]
    assert np.array_equal(lens, want[1]) and np.array_equal(counts, want[2])
    assert np.array_equal(proof, want[0]) and np.array_equal(out, want[3])
    ok, roots_out, hashed, bad = _verify(ctx, f, B, counts, out, proof, lens)
    want_hashed = sum(FR.range_counts(int(f.sizes[t]), int(a), int(a) + int(n), f.arity)[1] for t, a, n in zip(B.tid, B.first, np.diff(B.loff.astype(np.int64))))
    print("  verify: ok %d of %d, n_hashed %d (model %d), bad %d" % (int(ok.sum()), B.m, hashed, want_hashed, bad))
    assert (ok == 1).all() and bad == 0 and hashed == want_hashed
    assert np.array_equal(roots_out, f.roots[B.tid.astype(np.int64)])
    return proof, lens, counts, out


# ---- 1. one exhaustive call ----
@pytest.mark.parametrize("arity", [4, 2])
def test_every_run_of_the_small_trees_and_random_runs_of_the_others_in_one_call(gpu_ctx, arity):
    f = _forest(gpu_ctx, arity)
    rng = np.random.default_rng(arity)
    runs = [(t, a, b - a) for t, n in enumerate(SIZES) if n <= 17 for a in range(n) for b in range(a + 1, n + 1)]
    for _ in range(300):
        t = int(rng.integers(8, len(SIZES)))
        a = int(rng.integers(0, SIZES[t]))
        runs.append((t, a, int(rng.integers(1, SIZES[t] - a + 1))))
    order = rng.permutation(len(runs))  # (trees and lengths mixed: the dense lists' borders fall anywhere in the scan tiles)
    tid, first, lens = (np.array([runs[i][c] for i in order]) for c in range(3))
    B = Batch(tid, first, lens)
    assert B.m > 700 and B.m % 256 not in (0, 1)
    proof, plens, _, out = _round_trip(gpu_ctx, f, B)
    # the rows are the single-tree shared proofs of the same positions
    for r in rng.choice(B.m, size=32, replace=False):
        t, a, n = int(tid[r]), int(first[r]), int(lens[r])
        s_out, s_proof, s_len, s_bad = _single_extract(gpu_ctx, arity, SIZES[t], f.d[f.off[t]:f.off[t + 1]], f.d_lv[f.lo[t]:max(f.lo[t + 1], f.lo[t] + 1)],
                                                       np.arange(a, a + n))
        assert s_bad == 0 and s_len == int(plens[r]) and np.array_equal(s_proof[:s_len], proof[r, :s_len]), (t, a, n)
        assert not proof[r, s_len:].any() and np.array_equal(s_out, out[int(B.loff[r]):int(B.loff[r + 1])])
    # without d_leaves_out the proofs are the same
    again = _extract(gpu_ctx, f, B, int(B.loff[-1]), with_leaves=False)
    assert np.array_equal(again[0], proof) and np.array_equal(again[1], plens) and (again[3] == SENT64).all()


# ---- 2. past the 8-lane rule ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_long_run_past_the_lane_group_rule_beside_short_runs(gpu_ctx, arity):
    """131,077 leaves from an odd offset: levels 1 and up have more than 8,192 nodes, so their digests take the one-lane kernel; the
    three short runs of other trees share every launch"""
    f = _forest(gpu_ctx, arity, "large")
    B = Batch([1, 0, 3, 2], [3, 12345, 0, 1], [9, 131072 + 5, 64, 2])
    assert FR.level_bound(int(B.loff[-1]), B.m, 1, arity) > 8192
    _round_trip(gpu_ctx, f, B)


# ---- 3. whole trees ----
@pytest.mark.parametrize("arity", [4, 2])
def test_whole_trees_have_empty_proofs_and_hash_every_node(gpu_ctx, arity):
    import torch
    f = _forest(gpu_ctx, arity)
    B = Batch(np.arange(f.T), np.zeros(f.T), SIZES)
    proof, lens, counts, out = _round_trip(gpu_ctx, f, B)
    assert not lens.any() and not proof.any() and np.array_equal(out, f.leaves) and np.array_equal(counts, f.sizes.astype(np.uint64))
    ok, _, hashed, _ = _verify(gpu_ctx, f, B, counts, out, proof, lens)
    assert hashed == int(TS.levels_len(f.sizes, arity).sum()) and ok.all()
    # a stride of zero serves them: no proof buffer at all
    ok0 = torch.zeros(f.T, dtype=torch.uint8, device=f.d.device)
    call = gpu_ctx.merkle4_forest_range_verify_device if arity == 4 else gpu_ctx.merkle2_forest_range_verify_device
    call(_tag(arity), _torch(B.tid), _torch(counts), _torch(B.first), _torch(B.loff), B.m, f.top, f.d, f.n, None, 0, _torch(lens), f.d_roots, f.T, ok0)
    gpu_ctx.sync()
    assert bool(ok0.all())


# ---- 4. every kind of bad run, on both calls, with good neighbours ----
def _bad_batches(f):
    """{kind: (Batch, k, bad rows)} on the "bad tree" forest (sizes 5, 17, 0, 65, 1, 16)"""
    out = {}
    base = dict(tid=[0, 1, 3, 4, 5, 1], first=[1, 2, 10, 0, 4, 0], lens=[3, 10, 40, 1, 12, 17])

    def with_(row, **kw):
        v = {k: list(x) for k, x in base.items()}
        for key, val in kw.items():
            v[key][row] = val
        return Batch(v["tid"], v["first"], v["lens"]), int(sum(v["lens"]))
    out["tree id past the forest"] = with_(2, tid=6) + ([2],)
    out["tree id 2^32 - 1"] = with_(1, tid=0xFFFFFFFF) + ([1],)
    out["a bad tree"] = with_(2, tid=2, first=0, lens=1) + ([2],)
    out["one leaf too many"] = with_(1, first=8) + ([1],)
    out["first past the tree"] = with_(4, first=17, lens=1) + ([4],)
    out["first + len wraps"] = with_(2, first=2 ** 64 - 1, lens=2) + ([2],)
    out["first = 2^63"] = with_(0, first=2 ** 63) + ([0],)
    out["no leaf"] = with_(3, lens=0) + ([3],)
    k = sum(base["lens"])
    off = TS.offsets(base["lens"])
    dec = off.copy()
    dec[3] = dec[2] - 1  # run 2 decreases; run 3 then starts inside run 1 and is longer than its one-leaf tree
    out["decreasing offsets"] = (Batch(base["tid"], base["first"], leaf_offsets=dec), k, None)
    past = off.copy()
    past[-1] += 1
    out["past k"] = (Batch(base["tid"], base["first"], leaf_offsets=past), k, [5])
    huge = off.copy()
    huge[3:] = np.uint64(2 ** 64 - 5) + np.arange(4, dtype=np.uint64)
    out["offsets near 2^64"] = (Batch(base["tid"], base["first"], leaf_offsets=huge), k, [2, 3, 4, 5])
    return out


@pytest.mark.parametrize("arity", [4, 2])
def test_every_kind_of_bad_run_is_refused_alone_on_both_calls(gpu_ctx, oracle_mod, arity):
    f = _forest(gpu_ctx, arity, "bad tree")
    good = Batch([0, 1, 3, 4, 5, 1], [1, 2, 10, 0, 4, 0], [3, 10, 40, 1, 12, 17])
    g_proof, g_lens, g_counts, g_out = _round_trip(gpu_ctx, f, good)
    for kind, (B, k, rows) in _bad_batches(f).items():
        want = _model_extract(f, B, k)
        bad_rows = np.nonzero(want[1] == FR.BAD_LEN)[0].tolist()
        assert bad_rows and (rows is None or bad_rows == rows) and len(bad_rows) < B.m, (kind, bad_rows)
        proof, lens, counts, out, bad = _extract(gpu_ctx, f, B, k)
        print("%s: rows %s bad, device n_bad %d" % (kind, bad_rows, bad))
        assert bad == len(bad_rows) == want[4], kind
        assert np.array_equal(lens, want[1]) and np.array_equal(counts, want[2]) and np.array_equal(proof, want[0]) and np.array_equal(out, want[3]), kind
        assert not proof[bad_rows].any() and not counts[bad_rows].any()
        keep = [r for r in range(B.m) if r not in bad_rows]
        assert np.array_equal(proof[keep], g_proof[keep]) and np.array_equal(lens[keep], g_lens[keep])  # the neighbours are untouched
        # the verifier, given what this extraction returned (a count of 0 for a bad run) and the good batch's proofs and lengths
        leaves_in = np.where(out == SENT64, np.uint64(0), out)  # (no run reads what no run wrote)
        w_ok, w_roots, w_hashed, w_bad = _model_verify(oracle_mod, f, B, counts, leaves_in, g_proof, g_lens)
        ok, roots_out, hashed, bad = _verify(gpu_ctx, f, B, counts, leaves_in, g_proof, g_lens)
        assert np.array_equal(ok, w_ok) and (hashed, bad) == (w_hashed, w_bad), (kind, ok, w_ok, hashed, w_hashed, bad, w_bad)
        assert not ok[bad_rows].any() and ok[keep].all() and bad == len(bad_rows), kind
        for r in range(B.m):
            assert np.array_equal(roots_out[r], w_roots[r]) if r in w_roots else (roots_out[r] == SENT64).all(), (kind, r)
    # the verifier's own kinds: a claimed count of zero, above max_leaves, below the run's end
    for kind, row, count in (("count 0", 1, 0), ("count above max_leaves", 2, f.top + 1), ("count below the run's end", 4, 15), ("count 2^64 - 1", 0, 2 ** 64 - 1)):
        counts = g_counts.copy()
        counts[row] = np.uint64(count)
        w_ok, w_roots, w_hashed, w_bad = _model_verify(oracle_mod, f, good, counts, g_out, g_proof, g_lens)
        ok, roots_out, hashed, bad = _verify(gpu_ctx, f, good, counts, g_out, g_proof, g_lens)
        assert np.array_equal(ok, w_ok) and (hashed, bad) == (w_hashed, 1) and w_bad == 1, kind
        assert ok.sum() == good.m - 1 and ok[row] == 0 and (roots_out[row] == SENT64).all(), kind
    # a row stride too short for one run's proof: that run fails alone, and it is not a bad run
    short = int(g_lens.max()) - 1
    ok, roots_out, hashed, bad = _verify(gpu_ctx, f, good, g_counts, g_out, g_proof[:, :short], g_lens, stride=short)
    w_ok = _model_verify(oracle_mod, f, good, g_counts, g_out, g_proof[:, :short], g_lens)[0]
    assert np.array_equal(ok, w_ok) and bad == 0 and 0 < ok.sum() < good.m and np.array_equal(ok == 0, g_lens > short)


# ---- 5. every single change to one good batch ----
def _changes(f, B, counts, leaves, proof, lens, rng):
    """(what, row, changed (tid, counts, first, leaves, proof, lens, roots))"""
    base = dict(tid=B.tid, counts=counts, first=B.first, leaves=leaves, proof=proof, lens=lens, roots=f.roots)

    def change(what, row, **kw):
        v = dict(base)
        v.update(kw)
        return what, row, v

    def bump(name, row, by, dtype):
        a = base[name].copy()
        a[row] = dtype((int(a[row]) + by) % (1 << (8 * a.itemsize)))
        return a
    for r in range(B.m):
        for q in range(int(lens[r])):
            p = proof.copy()
            p[r, q, int(rng.integers(0, 4))] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 60)))
            yield change("proof scalar %d" % q, r, proof=p)
        lv = leaves.copy()
        lv[int(rng.integers(int(B.loff[r]), int(B.loff[r + 1]))), 0] ^= np.uint64(1)
        yield change("a leaf", r, leaves=lv)
        for by in (1, -1):
            yield change("first %+d" % by, r, first=bump("first", r, by, np.uint64))
            yield change("count %+d" % by, r, counts=bump("counts", r, by, np.uint64))
            yield change("proof_len %+d" % by, r, lens=bump("lens", r, by, np.uint32))
        yield change("the tree id", r, tid=bump("tid", r, 1, np.uint32))
        roots = f.roots.copy()
        roots[int(B.tid[r]), 3] ^= np.uint64(1)
        yield change("the root", r, roots=roots)
        if int(lens[r]) >= 2:
            p = proof.copy()
            p[r, [0, 1]] = p[r, [1, 0]]
            yield change("swapped siblings", r, proof=p)


@pytest.mark.parametrize("arity", [4, 2])
def test_every_single_change_to_a_good_batch_gives_the_models_byte(gpu_ctx, oracle_mod, arity):
    """the changed row's byte is the model's — 0 but for a changed count that leaves every w_l on the run's path alone —, and the
    unchanged rows stay 1 (a changed root fails every run of that tree: none shares one here)"""
    f = _forest(gpu_ctx, arity)
    B = Batch([4, 7, 10, 11, 0, 6, 8], [1, 5, 20, 100, 0, 4, 0], [3, 9, 33, 57, 1, 8, 60])
    assert len(set(B.tid.tolist())) == B.m
    proof, lens, counts, out = _round_trip(gpu_ctx, f, B)
    n, passed, rng = 0, [], np.random.default_rng(5 + arity)
    for what, row, v in _changes(f, B, counts, out, proof, lens, rng):
        C = Batch(v["tid"], v["first"], leaf_offsets=B.loff)
        w_ok, _, w_hashed, w_bad = _model_verify(oracle_mod, f, C, v["counts"], v["leaves"], v["proof"], v["lens"], roots=v["roots"])
        ok, _, hashed, bad = _verify(gpu_ctx, f, C, v["counts"], v["leaves"], v["proof"], v["lens"], roots=v["roots"])
        assert np.array_equal(ok, w_ok) and (hashed, bad) == (w_hashed, w_bad), (what, row, ok, w_ok, hashed, w_hashed, bad, w_bad)
        assert all(ok[r] == 1 for r in range(B.m) if r != row), (what, row, ok)
        if ok[row]:
            passed.append((what, row))
        n += 1
    print("arity %d: %d changes, passed: %s" % (arity, n, passed))
    assert n == int(lens.sum()) + 9 * B.m + int((lens >= 2).sum())  # each proof scalar; a leaf, six +-1, the tree id, the root; the swap
    assert passed and all(what.startswith("count") for what, _ in passed)


# ---- 6. leaves at and above the modulus ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_leaf_above_the_modulus_verifies_and_a_lone_one_follows_the_mod_p_rule(gpu_ctx, arity):
    P = E.P
    leaves = _leaves(1 + 9 + 1 + 1, 77)
    leaves[0] = E.limbs(P + 1)  # the one-leaf tree
    leaves[4] = E.limbs(P + 1)  # leaf 3 of the nine-leaf tree
    leaves[10] = E.limbs(2 * P + 5)  # one-leaf trees whose leaves take two subtractions, and none
    leaves[11] = E.limbs(P - 1)
    f = Forest(gpu_ctx, arity, [1, 9, 1, 1], leaves)
    assert np.array_equal(f.roots[0], np.array(E.limbs(1), dtype=np.uint64))  # the forest's convention
    assert np.array_equal(f.roots[2], np.array(E.limbs(5), dtype=np.uint64)) and np.array_equal(f.roots[3], leaves[11])
    B = Batch([0, 1, 2, 3], [0, 2, 0, 0], [1, 4, 1, 1])
    proof, lens, counts, out = _round_trip(gpu_ctx, f, B)
    assert np.array_equal(out[0], leaves[0]) and np.array_equal(out[2], leaves[4])  # byte for byte, not reduced
    reduced = out.copy()
    reduced[[0, 2]] = np.array(E.limbs(1), dtype=np.uint64)
    ok, roots_out, _, _ = _verify(gpu_ctx, f, B, counts, reduced, proof, lens)
    assert ok.all() and np.array_equal(roots_out, f.roots)
    other = out.copy()
    other[0] = E.limbs(P + 2)
    ok, roots_out, _, _ = _verify(gpu_ctx, f, B, counts, other, proof, lens)
    assert ok.tolist() == [0, 1, 1, 1] and np.array_equal(roots_out[0], np.array(E.limbs(2), dtype=np.uint64))


# ---- 7. two streams of one context ----
def test_two_streams_of_one_context_give_what_one_gives(gpu_ctx):
    import torch
    f = _forest(gpu_ctx, 4)
    rng = np.random.default_rng(12)
    batches = []
    for s in range(2):
        tid = rng.integers(5, len(SIZES), size=40 + 300 * s)
        first = np.array([rng.integers(0, SIZES[t]) for t in tid])
        lens = np.array([rng.integers(1, SIZES[t] - a + 1) for t, a in zip(tid, first)])
        batches.append(Batch(tid, first, lens))
    alone = [_round_trip(gpu_ctx, f, B) for B in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    held, outs = [], []
    for B, st in zip(batches, streams):  # both calls of both batches are queued before anything is read
        with torch.cuda.stream(st):
            st.wait_stream(torch.cuda.default_stream())
            k = int(B.loff[-1])
            dev = f.d.device
            t = dict(tid=_torch(B.tid), first=_torch(B.first), loff=_torch(B.loff), proof=torch.zeros((B.m, f.stride, 4), dtype=torch.int64, device=dev),
                     lens=torch.zeros(B.m, dtype=torch.int32, device=dev), counts=torch.zeros(B.m, dtype=torch.int64, device=dev),
                     out=torch.zeros((k, 4), dtype=torch.int64, device=dev), ok=torch.zeros(B.m, dtype=torch.uint8, device=dev),
                     roots=torch.zeros((B.m, 4), dtype=torch.int64, device=dev), hashed=torch.zeros(1, dtype=torch.int64, device=dev))
            gpu_ctx.merkle4_forest_ragged_range_proofs_device(f.d, f.d_off, f.T, f.top, f.d_lv, t["tid"], t["first"], t["loff"], B.m, k, t["proof"], t["lens"],
                                                              t["counts"], d_leaves_out=t["out"])
            gpu_ctx.merkle4_forest_range_verify_device(_tag(4), t["tid"], t["counts"], t["first"], t["loff"], B.m, f.top, t["out"], k, t["proof"], f.stride,
                                                       t["lens"], f.d_roots, f.T, t["ok"], d_roots_out=t["roots"], d_n_hashed=t["hashed"])
            held.append(t)
    torch.cuda.synchronize()
    for B, t, (proof, lens, counts, out) in zip(batches, held, alone):
        assert np.array_equal(_np(t["proof"]), proof) and np.array_equal(_np(t["lens"]).view(np.uint32), lens) and np.array_equal(_np(t["out"]), out)
        assert bool(t["ok"].all()) and np.array_equal(_np(t["roots"]), f.roots[B.tid.astype(np.int64)])
    # the scratch of both streams is the context's: trimmed, the same bytes again
    gpu_ctx.trim()
    again = _round_trip(gpu_ctx, f, batches[0])
    assert all(np.array_equal(x, y) for x, y in zip(again, alone[0]))


# ---- 8. the conveniences ----
@pytest.mark.parametrize("arity", [4, 2])
def test_the_conveniences_prove_and_verify_runs_given_as_sequences(gpu_ctx, arity):
    import poseidon252_amd as P
    import torch
    f = _forest(gpu_ctx, arity)
    tid, first, lens = [11, 0, 7, 11], [3, 0, 0, 200], [100, 1, 17, 57]
    r_t, r_first, r_off, leaves, proof, plens, counts = P.forest_ragged_range_proofs(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, tid, first, lens, arity=arity)
    assert proof.shape == (4, P.forest_range_stride(f.top, arity), 4) == (4, f.stride, 4) and leaves.shape == (sum(lens), 4)
    want = _model_extract(f, Batch(tid, first, lens), sum(lens))
    assert np.array_equal(_np(proof), want[0]) and np.array_equal(_np(plens).view(np.uint32), want[1]) and np.array_equal(_np(leaves), want[3])
    assert _np(r_off).tolist() == TS.offsets(lens).tolist() and _np(counts).tolist() == [257, 1, 17, 257]
    ok = P.forest_range_verify(gpu_ctx, r_t, counts, r_first, r_off, leaves, proof, plens, f.d_roots, f.top, arity=arity)
    assert ok.dtype == torch.bool and ok.tolist() == [True] * 4
    leaves[5, 0] ^= 1
    assert P.forest_range_verify(gpu_ctx, r_t, counts, r_first, r_off, leaves, proof, plens, f.d_roots, f.top, arity=arity).tolist() == [False, True, True, True]
    # refused before the call (an id past the forest, a negative first leaf, an empty run) or by it (a run past its tree's leaves)
    for t, a, n in (([12, 0, 7, 11], first, lens), (tid, [-1, 0, 0, 0], lens), (tid, first, [100, 0, 17, 57]), (tid, [200, 0, 0, 200], lens)):
        with pytest.raises(ValueError, match="outside the forest"):
            P.forest_ragged_range_proofs(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, t, a, n, arity=arity)
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        P.forest_ragged_range_proofs(gpu_ctx, f.d, f.d_off, f.T, f.top, f.d_lv, tid, first, lens, arity=3)
