"""Consistency proofs of a ragged forest — that a grown tree extends its old root (p252_merkle{4,2}_forest_ragged_consistency_device_into
and _forest_consistency_verify_device_into; csrc/forest_consistency.hip) on the GPU.  The references are the oracle's builds of
leaves[:n] and leaves[:m], the openings call, and the numpy model (testsupport/forestconsistency.py, checked against the oracle
without a GPU) — never the calls themselves: every pair of small counts with the bad ones; every single change to a good proof;
forests whose old leaf was altered before they grew; thousands of proofs over many blocks and depth bins, sorted and not; the
hand-over from a frontier state to a grown forest on a side stream; the C++ mirror and the refusal program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from testsupport import forestconsistency as FC
from testsupport import forestfrontier as FF
from testsupport import treeshape as TS
from helpers.forest import Old, SENTINEL, _np, _tag, _torch, _tree
from helpers.percall import assert_rows_equal_golden, build_cpp_mirror, refusal_table, run_cpp_mirror

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
TOP = {4: 70, 2: 40}
MAX_LEAVES = {4: 1024, 2: 128}  # the stride exceeds every depth
TAIL = 3


def _extract(ctx, arity, f, tid, old):
    """one extraction of the proofs (tid, old) out of the built forest f (an Old) into canary-tailed buffers -> dict of numpy results"""
    import torch
    k, D = len(tid), TS.depth(f.max_leaves, arity)
    full = lambda shape, fill, dtype: torch.full(shape, fill, dtype=dtype, device="cuda:0")  # noqa: E731
    bufs = [full((k + TAIL,), SENTINEL, torch.int64), full((k + TAIL, 4), SENTINEL, torch.int64), full((k + TAIL, D, arity - 1, 4), SENTINEL, torch.int64),
            full((k + TAIL, D), CANARY, torch.uint8), full((k + TAIL,), CANARY, torch.uint8)]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    call = ctx.merkle4_forest_ragged_consistency_device if arity == 4 else ctx.merkle2_forest_ragged_consistency_device
    call(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(old, np.uint64)), k,
         *(b[:k] for b in bufs), bad)
    torch.cuda.synchronize()
    intact = all(bool((b[k:] == fill).all()) for b, fill in zip(bufs, (SENTINEL, SENTINEL, SENTINEL, CANARY, CANARY)))
    newc, lv, sib, pos, dep = (_np(b[:k]) for b in bufs)
    return dict(newc=newc, lv=lv, sib=sib, pos=pos, dep=dep, bad=int(bad), intact=intact, D=D)


def _verify(ctx, arity, D, n, old_roots, m, new_roots, lv, sib, pos, dep, tree_ids=None, n_trees=0):
    """one verification of numpy inputs -> (ok, old roots out, new roots out, digests), the outputs' canary tails checked"""
    import torch
    k = len(dep)
    ok = torch.full((k + TAIL,), 7, dtype=torch.uint8, device="cuda:0")
    old_out, new_out = (torch.full((k + TAIL, 4), SENTINEL, dtype=torch.int64, device="cuda:0") for _ in range(2))
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    u64 = lambda a: _torch(np.ascontiguousarray(a, dtype=np.uint64))  # noqa: E731
    call = ctx.merkle4_forest_consistency_verify_device if arity == 4 else ctx.merkle2_forest_consistency_verify_device
    call(_tag(arity), u64(n), u64(old_roots), u64(m), u64(new_roots), u64(lv), u64(sib), _torch(np.ascontiguousarray(pos, dtype=np.uint8)),
         _torch(np.ascontiguousarray(dep, dtype=np.uint8)), D, k, ok[:k], None if tree_ids is None else _torch(np.asarray(tree_ids, np.uint32)), n_trees,
         old_out[:k], new_out[:k], hashed)
    torch.cuda.synchronize()
    assert bool((ok[k:] == 7).all()) and bool((old_out[k:] == SENTINEL).all()) and bool((new_out[k:] == SENTINEL).all())
    return ok[:k].cpu().numpy(), _np(old_out[:k]), _np(new_out[:k]), int(hashed)


def _model_arrays(proofs):
    """[leaves, siblings, positions, depths] of a list of model proofs"""
    return [np.array([p.leaf for p in proofs]), np.array([p.siblings for p in proofs]), np.array([p.positions for p in proofs]),
            np.array([p.depth for p in proofs], dtype=np.uint8)]


# ---- 1, 2. every pair of small counts ----
@pytest.fixture(scope="module", params=[4, 2])
def pairs(request, gpu_ctx, oracle_mod):
    """one forest of trees of 1 .. 70 (arity 2: 40) leaves and an empty tree, every tree a prefix of the same leaves so that the oracle
    builds each count once; every (t, n) with 1 <= n <= n_t, and the bad ones: n == 0 and n == n_t + 1 of every tree, tree ids out of
    range, the empty tree.  The extraction is run once here; test 1 checks it and test 2 changes it."""
    arity = request.param
    top, max_leaves = TOP[arity], MAX_LEAVES[arity]
    leaves = oracle_mod.fill_random(0xC70 + arity, top)
    built = {n: _tree(oracle_mod, arity)(_tag(arity), leaves[:n], want_levels=True)[:2] for n in range(1, top + 1)}
    root = lambda n: FF.reduce_leaf(leaves[0]) if n == 1 else built[n][0]  # noqa: E731
    sizes = list(range(1, top + 1)) + [0]
    T = len(sizes)
    f = Old(gpu_ctx, arity, np.concatenate([leaves[:n] for n in sizes if n]), TS.offsets(sizes), max_leaves)
    tid = [t for t in range(top) for _ in range(sizes[t])]
    old = [n for t in range(top) for n in range(1, sizes[t] + 1)]
    for t in range(top):
        tid += [t, t]
        old += [0, sizes[t] + 1]
    tid += [T, T + 5, T - 1, T - 1, 2 ** 32 - 1]
    old += [1, 3, 1, 0, 1]
    order = np.random.default_rng(arity).permutation(len(tid))
    tid, old = np.asarray(tid, dtype=np.int64)[order], np.asarray(old, dtype=np.int64)[order]
    m = np.array([sizes[t] if t < T else 0 for t in tid], dtype=np.int64)
    good = (old >= 1) & (old <= m)
    D = TS.depth(max_leaves, arity)
    model = [FC.proof_of(leaves, built[int(mm)][1] if mm else None, int(mm), int(nn), arity, D) for nn, mm in zip(old, m)]
    zero = np.zeros(4, dtype=np.uint64)
    old_roots = np.array([root(int(nn)) if g else zero for nn, g in zip(old, good)])
    new_roots = np.array([root(int(mm)) if g else zero for mm, g in zip(m, good)])
    got = _extract(gpu_ctx, arity, f, tid, old)
    return dict(arity=arity, f=f, tid=tid, old=old, m=m, good=good, grown=good & (old < m), D=D, model=model, old_roots=old_roots, new_roots=new_roots,
                got=got, sizes=sizes)


def test_every_pair_of_small_counts_and_the_bad_ones(gpu_ctx, oracle_mod, pairs):
    """the extraction byte for byte the model's and — where there is a leaf n to open — the openings call's; canaries, the bad count;
    verdict 1 for every good proof and 0 for every bad one; both roots out the oracle's builds; the digest count the model's"""
    import torch
    p, arity, got = pairs, pairs["arity"], pairs["got"]
    k = len(p["tid"])
    assert k > 2 * 256 and p["D"] > max(TS.depth(n, arity) for n in p["sizes"])
    want = _model_arrays([w for w, _ in p["model"]])
    for name, w in zip(("lv", "sib", "pos", "dep"), want):
        assert np.array_equal(got[name], w.reshape(got[name].shape)), name
    assert np.array_equal(got["newc"].astype(np.int64), np.array([c for _, c in p["model"]])) and np.array_equal(got["newc"].astype(np.int64), np.where(p["good"], p["m"], 0))
    assert got["intact"] and got["bad"] == int((~p["good"]).sum()) and int((~p["good"]).sum()) == 2 * TOP[arity] + 5
    assert (got["dep"][~p["good"]] == 0xFF).all() and np.array_equal(got["dep"][p["good"]], TS.depth(p["m"][p["good"]], arity).astype(np.uint8))
    same = p["good"] & ~p["grown"]
    assert same.sum() == TOP[arity] and not got["lv"][~p["grown"]].any() and not got["sib"][~p["grown"]].any() and not got["pos"][~p["grown"]].any()
    # the openings call of (t, leaf n)
    f, g = p["f"], p["grown"]
    lv, sib, pos, dep, _ = gpu_ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, _torch(p["tid"][g].astype(np.uint32)),
                                                                        _torch(p["old"][g].astype(np.uint64)), int(g.sum()), arity=arity)
    torch.cuda.synchronize()
    for name, o in zip(("lv", "sib", "pos", "dep"), (lv, sib, pos, dep)):
        assert np.array_equal(got[name][g], _np(o)), name
    # the verification
    ok, old_out, new_out, hashed = _verify(gpu_ctx, arity, p["D"], p["old"], p["old_roots"], got["newc"], p["new_roots"], got["lv"], got["sib"], got["pos"],
                                           got["dep"])
    assert np.array_equal(ok, p["good"].astype(np.uint8))
    assert np.array_equal(old_out, p["old_roots"]) and np.array_equal(new_out, p["new_roots"])  # (zero for the bad ones)
    assert hashed == sum(FC.n_hashed(int(n), int(m), arity) for n, m in zip(p["old"][g], p["m"][g]))
    assert np.array_equal(_np(f.roots)[:TOP[arity]][1:], np.array([p["new_roots"][(p["m"] == n) & p["good"]][0] for n in range(2, TOP[arity] + 1)]))


def _flip(a, rng):
    """one random bit of the scalar a (4 uint64 limbs), in place"""
    b = int(rng.integers(0, 256))
    a[b // 64] ^= np.uint64(1) << np.uint64(b % 64)


def test_every_single_change_to_a_good_proof_is_refused(gpu_ctx, pairs):
    """each change is made to EVERY proof it applies to, in one call; the others stay as they were, and their verdicts too.  n + 1, n - 1,
    the depth byte, the roots and the swap apply to every good proof (the swap to those with n < m: for n == m it changes nothing); the
    bit flips and the position byte to those with n < m, whose opening is read; a right sibling exists unless n = A^depth(m) - 1.
    m + 1 applies where it changes the depth, or makes an unchanged tree a grown one: elsewhere (n, old root, m + 1, new root) IS a true
    statement — about the tree followed by a zero leaf, whose root is the same — and no verifier can refuse it."""
    p, arity, got = pairs, pairs["arity"], pairs["got"]
    A, D, k = arity, p["D"], len(p["tid"])
    good, grown = p["good"], p["grown"]
    n0, m0 = p["old"], got["newc"].astype(np.int64)
    dm = TS.depth(p["m"], arity)
    digit = lambda n, l: n // A ** l % A  # noqa: E731
    rng = np.random.default_rng(50 + arity)

    def run(n=None, m=None, old_roots=None, new_roots=None, lv=None, sib=None, pos=None, dep=None):
        pick = lambda x, base: base if x is None else x  # noqa: E731
        return _verify(gpu_ctx, arity, D, pick(n, n0), pick(old_roots, p["old_roots"]), pick(m, m0), pick(new_roots, p["new_roots"]), pick(lv, got["lv"]),
                       pick(sib, got["sib"]), pick(pos, got["pos"]), pick(dep, got["dep"]))[0]

    def check(ok, applies, what):
        assert applies.any(), what
        assert not ok[applies].any(), (what, np.nonzero(ok.astype(bool) & applies)[0][:8])
        assert np.array_equal(ok[~applies], good[~applies].astype(np.uint8)), what
    # a left sibling of a row with d_l(n) > 0
    sib = got["sib"].copy()
    for i in np.nonzero(grown)[0]:
        rows = [l for l in range(dm[i]) if digit(n0[i], l) > 0]
        l = rows[int(rng.integers(len(rows)))]
        _flip(sib[i, l, int(rng.integers(digit(n0[i], l)))], rng)
    check(run(sib=sib), grown, "left sibling")
    # a right sibling of a row below depth(m)
    sib, applies = got["sib"].copy(), np.zeros(k, dtype=bool)
    for i in np.nonzero(grown)[0]:
        rows = [l for l in range(dm[i]) if digit(n0[i], l) < A - 1]
        if rows:
            l = rows[int(rng.integers(len(rows)))]
            _flip(sib[i, l, int(rng.integers(digit(n0[i], l), A - 1))], rng)
            applies[i] = True
    assert all(n0[i] == A ** dm[i] - 1 for i in np.nonzero(grown & ~applies)[0]) and (grown & ~applies).sum() >= 2
    check(run(sib=sib), applies, "right sibling")
    # a row at or past depth(m) is not read
    sib = got["sib"].copy()
    for i in np.nonzero(grown)[0]:
        _flip(sib[i, int(rng.integers(dm[i], D)), int(rng.integers(A - 1))], rng)
    assert np.array_equal(run(sib=sib), good.astype(np.uint8))
    # the leaf, the roots
    lv = got["lv"].copy()
    for i in np.nonzero(grown)[0]:
        _flip(lv[i], rng)
    check(run(lv=lv), grown, "leaf")
    for name in ("old_roots", "new_roots"):
        roots = p[name].copy()
        for i in np.nonzero(good)[0]:
            _flip(roots[i], rng)
        check(run(**{name: roots}), good, name)
    # a position byte
    pos = got["pos"].copy()
    for i in np.nonzero(grown)[0]:
        pos[i, int(rng.integers(dm[i]))] ^= np.uint8(1 << int(rng.integers(0, 2 if A == 4 else 1)))
    check(run(pos=pos), grown, "position")
    # the depth byte
    for delta in (1, -1, None):
        dep = got["dep"].copy()
        dep[good] = 0xFF if delta is None else (dep[good].astype(np.int64) + delta) % 256
        check(run(dep=dep), good, ("depth", delta))
    # the counts
    for delta in (1, -1):
        n = n0.copy()
        n[good] += delta
        check(run(n=n), good, ("n", delta))
    m = m0.copy()
    m[good] += 1
    changes_depth = TS.depth(p["m"] + 1, arity) != dm
    applies = good & (changes_depth | ~grown)
    ok = run(m=m)
    check(ok, applies, "m + 1")
    assert (good & ~applies).sum() > 500 and ok[good & ~applies].all()
    n, m = n0.copy(), m0.copy()
    n[grown], m[grown] = m0[grown], n0[grown]
    check(run(n=n, m=m), grown, "swap")


# ---- 3. forks ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_forest_whose_old_leaf_was_altered_before_it_grew(gpu_ctx, oracle_mod, arity):
    """every n <= m <= 20 and j in {0, n - 1}: the trees with leaf j altered are built on the device and the proofs extracted honestly
    from them; against the honest old root the verdict is 0 — and 1 against the forked tree's own old root, so the proof itself is sound"""
    top, max_leaves = 20, 64
    leaves, other = oracle_mod.fill_random(0xC80 + arity, top), oracle_mod.fill_random(0xC90 + arity, top)
    honest = {n: FF.reduce_leaf(leaves[0]) if n == 1 else _tree(oracle_mod, arity)(_tag(arity), leaves[:n])[0] for n in range(1, top + 1)}
    trees, tid, old = [], [], []
    for j in range(top):
        for m in range(j + 1, top + 1):
            forked = leaves[:m].copy()
            forked[j] = other[j]
            for n in (range(1, m + 1) if j == 0 else [j + 1]):
                tid.append(len(trees)), old.append(n)
            trees.append(forked)
    assert len(tid) == 2 * 210 - top
    f = Old(gpu_ctx, arity, np.concatenate(trees), TS.offsets([t.shape[0] for t in trees]), max_leaves)
    got = _extract(gpu_ctx, arity, f, tid, old)
    assert got["bad"] == 0 and got["intact"]
    tid, old = np.asarray(tid), np.asarray(old)
    new_roots = _np(f.roots)[tid]
    old_roots = np.array([honest[int(n)] for n in old])
    ok, old_out, new_out, _ = _verify(gpu_ctx, arity, got["D"], old, old_roots, got["newc"], new_roots, got["lv"], got["sib"], got["pos"], got["dep"])
    assert not ok.any()
    grown = old < got["newc"].astype(np.int64)
    assert np.array_equal(new_out[grown], new_roots[grown]) and (old_out[grown] != old_roots[grown]).any(axis=1).all()
    own = np.where(grown[:, None], old_out, new_roots)
    assert _verify(gpu_ctx, arity, got["D"], old, own, got["newc"], new_roots, got["lv"], got["sib"], got["pos"], got["dep"])[0].all()


# ---- 4. width ----
BIG = 4 ** 6 + 5
BIG_COUNTS = (1, 4 ** 5, 4 ** 5 + 1, 4 ** 6 - 1, 4 ** 6, 4 ** 6 + 4, 4 ** 6 + 5)

_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import poseidon252_amd as P
from poseidon252_amd import merkle
from helpers.forest import Old, _np, _torch
z = np.load(%r)
arity = int(z["arity"])
ctx = P.Context(0)
f = Old(ctx, arity, z["flat"], z["off"], int(z["max_leaves"]))
newc, (lv, sib, pos, dep, D), bad = merkle.forest_ragged_consistency(ctx, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, z["tid"], z["old"], arity=arity)
ok, old_out, new_out, hashed = merkle.forest_consistency_verify(ctx, _torch(z["old"].astype(np.uint64)), _torch(z["old_roots"]), newc, _torch(z["new_roots"]),
                                                                (lv, sib, pos, dep, D), arity=arity)
torch.cuda.synchronize()
np.savez(%r, newc=_np(newc), lv=_np(lv), sib=_np(sib), pos=_np(pos), dep=_np(dep), bad=int(bad), ok=ok.cpu().numpy(), old_out=_np(old_out),
         new_out=_np(new_out), hashed=int(hashed))
print("done")
"""


@pytest.mark.parametrize("arity", [4, 2])
def test_many_blocks_and_depth_bins_sorted_and_unsorted(gpu_ctx, oracle_mod, tmp_path, arity):
    """300 trees of 1 .. 600 leaves with 5,000 random (t, n) proofs, and one tree of 4^6 + 5 leaves with n = 1, 4^5, 4^5 + 1, 4^6 - 1,
    4^6, 4^6 + 4 and 4^6 + 5, in one forest: against the model (the proofs cut out of the oracle's builds, the roots from the model's
    two chains), in this process with the depth sort and in a fresh child process under P252_RAGGED_SORT=0 (read once per process)"""
    rng = np.random.default_rng(0xC0 + arity)
    sizes = [int(x) for x in rng.integers(1, 601, 300)] + [BIG]
    off = TS.offsets(sizes, dtype=np.int64)
    flat = oracle_mod.fill_random(0xCA0 + arity, int(off[-1]))
    built = [_tree(oracle_mod, arity)(_tag(arity), flat[off[t]:off[t + 1]], want_levels=True)[:2] for t in range(len(sizes))]
    tid = np.concatenate([rng.integers(0, 300, 5000), np.full(len(BIG_COUNTS), 300)])
    old = np.concatenate([1 + (rng.random(5000) * np.asarray(sizes)[tid[:5000]]).astype(np.int64), np.asarray(BIG_COUNTS)])
    m = np.asarray(sizes)[tid]
    assert (old >= 1).all() and (old <= m).all() and (old == m).sum() >= 2
    D = TS.depth(BIG, arity)
    model = [FC.proof_of(flat[off[t]:off[t + 1]], built[t][1], int(mm), int(nn), arity, D)[0] for t, nn, mm in zip(tid, old, m)]
    want = _model_arrays(model)
    assert len(set(want[3].tolist())) >= 4  # several depth bins
    grown = old < m
    new_roots = np.array([FF.reduce_leaf(flat[off[t]]) if sizes[t] == 1 else built[t][0] for t in tid])
    old_g, new_g, hashed = FC.roots_many(want[0][grown], want[1][grown], old[grown], m[grown], lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1), arity)
    assert np.array_equal(new_g, new_roots[grown])
    old_roots = new_roots.copy()  # (an unchanged tree: its root)
    old_roots[grown] = old_g
    # the old roots of the large tree, against the oracle's builds of its first n leaves
    for i in range(5000, len(tid)):
        if grown[i] and old[i] > 1:
            assert np.array_equal(old_roots[i], _tree(oracle_mod, arity)(_tag(arity), flat[off[300]:off[300] + old[i]])[0]), old[i]

    def check(r, what):
        for name, w in zip(("lv", "sib", "pos", "dep"), want):
            assert np.array_equal(r[name], w.reshape(r[name].shape)), (what, name)
        assert np.array_equal(np.asarray(r["newc"]).astype(np.int64), m) and int(r["bad"]) == 0, what
        assert np.asarray(r["ok"]).all(), (what, np.nonzero(np.asarray(r["ok"]) == 0)[0][:8])
        assert np.array_equal(r["old_out"], old_roots) and np.array_equal(r["new_out"], new_roots) and int(r["hashed"]) == hashed, what
    f = Old(gpu_ctx, arity, flat, off.astype(np.uint64), BIG)
    got = _extract(gpu_ctx, arity, f, tid, old)
    assert got["intact"]
    ok, old_out, new_out, n_hashed = _verify(gpu_ctx, arity, D, old, old_roots, got["newc"], new_roots, got["lv"], got["sib"], got["pos"], got["dep"])
    check(dict(got, ok=ok, old_out=old_out, new_out=new_out, hashed=n_hashed), "sorted")
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, arity=arity, flat=flat, off=off.astype(np.uint64), max_leaves=BIG, tid=tid, old=old, old_roots=old_roots, new_roots=new_roots)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), src, dst)], env=dict(os.environ, P252_RAGGED_SORT="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    check(np.load(dst), "unsorted")


# ---- 5. the hand-over ----
@pytest.mark.parametrize("arity", [4, 2])
def test_hand_over_from_a_frontier_state_to_the_grown_forest_on_a_side_stream(gpu_ctx, oracle_mod, arity):
    """an auditor holds the ForestFrontier of a forest; the publisher appends (stored) and extracts one proof per tree with the state's
    counts as the old counts; the auditor verifies with the state's (counts, roots) as the old claims and the grown forest's as the new
    ones, by tree id, with no gather — and then reaches the same roots by appending the same leaves to the state"""
    import torch
    from poseidon252_amd import merkle
    sizes, adds = [3, 1, 17, 64, 5, 16], [2, 0, 47, 1, 11, 48]
    T = len(sizes)
    flat, add = oracle_mod.fill_random(0xCB0 + arity, sum(sizes)), oracle_mod.fill_random(0xCC0 + arity, sum(adds))
    off, aoff = TS.offsets(sizes, dtype=np.int64), TS.offsets(adds, dtype=np.int64)
    old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), 64)
    state, _ = merkle.ForestFrontier.from_forest(gpu_ctx, old.d, old.d_off, T, 64, old.d_lv, old.roots, max_leaves=100, arity=arity)
    d_add, d_aoff = _torch(add), _torch(TS.offsets(adds))
    ids = torch.arange(T, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g_leaves, g_off, g_lv, g_roots, g_bad, _ = merkle.forest_ragged_append(gpu_ctx, _tag(arity), old.d, old.d_off, T, 64, old.d_lv, d_add, d_aoff,
                                                                               max_leaves_new=100, arity=arity)
        new_counts, proof, n_bad = merkle.forest_ragged_consistency(gpu_ctx, g_leaves, g_off, T, 100, g_lv, ids, state.counts, arity=arity)
        g_counts = (g_off[1:] - g_off[:-1]).contiguous()
        ok, old_out, new_out, hashed = merkle.forest_consistency_verify(gpu_ctx, state.counts, state.roots, g_counts, g_roots, proof, d_tree_ids=ids,
                                                                        arity=arity)
        side.synchronize()
        assert int(g_bad) == 0 and int(n_bad) == 0 and torch.equal(new_counts, g_counts) and g_counts.tolist() == [n + a for n, a in zip(sizes, adds)]
        assert ok.tolist() == [1] * T and torch.equal(old_out, state.roots) and torch.equal(new_out, g_roots)
        assert int(hashed) == sum(FC.n_hashed(n, n + a, arity) for n, a in zip(sizes, adds))
        assert proof[3].tolist() == [int(TS.depth(n + a, arity)) for n, a in zip(sizes, adds)] and not proof[1][1].any()  # (tree 1 did not grow)
        # a stale auditor (one tree's count off by one) is refused for that tree alone
        stale = state.counts.clone()
        stale[2] -= 1
        ok2 = merkle.forest_consistency_verify(gpu_ctx, stale, state.roots, g_counts, g_roots, proof, d_tree_ids=ids, arity=arity)[0]
        state.append(d_add, d_aoff)
        side.synchronize()
        assert ok2.tolist() == [1, 1, 0, 1, 1, 1]
        assert torch.equal(state.roots, g_roots) and torch.equal(state.counts, g_counts)
    torch.cuda.synchronize()
    for t in (0, 2, 5):
        grown = np.concatenate([flat[off[t]:off[t + 1]], add[aoff[t]:aoff[t + 1]]])
        assert np.array_equal(_np(g_roots)[t], _tree(oracle_mod, arity)(_tag(arity), grown)[0]), t


def test_trivial_sizes(gpu_ctx, oracle_mod):
    """max_leaves == 1 has no rows: every proof is an unchanged one-leaf tree or a bad one"""
    import torch
    for arity in (4, 2):
        leaves = oracle_mod.fill_random(0xCD0 + arity, 3)
        f = Old(gpu_ctx, arity, leaves, np.array([0, 1, 2, 3], dtype=np.uint64), 1)
        got = _extract(gpu_ctx, arity, f, [0, 2, 1, 3, 1], [1, 1, 2, 1, 0])
        assert got["D"] == 0 and got["bad"] == 3 and got["intact"] and got["dep"].tolist() == [0, 0, 0xFF, 0xFF, 0xFF] and got["newc"].tolist() == [1, 1, 0, 0, 0]
        assert not got["lv"].any()
        roots = _np(f.roots)[[0, 2, 1, 0, 1]]
        ok, old_out, new_out, hashed = _verify(gpu_ctx, arity, 0, [1, 1, 2, 1, 0], roots, got["newc"], roots, got["lv"], np.zeros((5, 0, arity - 1, 4), np.uint64),
                                               np.zeros((5, 0), np.uint8), got["dep"])
        assert ok.tolist() == [1, 1, 0, 0, 0] and hashed == 0 and np.array_equal(old_out[:2], roots[:2]) and not old_out[2:].any() and not new_out[2:].any()
        torch.cuda.synchronize()


# ---- 6. the mirrors ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_consistency_api", tmp_path))


def test_refusal_program_on_gpu(gpu_ctx, tmp_path):
    assert_rows_equal_golden(refusal_table("consistency_refusal_table", tmp_path), "consistency_refusals")
