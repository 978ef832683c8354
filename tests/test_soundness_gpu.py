"""Every single change to a good proof, put to every Merkle verifier on the GPU: p252_merkle{4,2}_multiproof_verify_device,
_forest_ragged_multiproof_verify_device_into, _verify_batch_device and _forest_ragged_verify_device (on the build's openings and on
anchored ones).  The cases and the verdicts are tests/soundcases.py's — the catalogue of testsupport/soundness.py on the oracle's trees,
judged by the numpy models, never by the calls themselves; tests/test_soundness_cpu.py shows that the catalogue would notice a wrong
verifier.  Every verdict, recomputed root and count must be the model's; every output has a canary tail; a good call afterwards still
verifies.  Which digest kernel a shared-proof call reaches follows from its level bounds (multiproof.hip mp_digests, forest_multiproof.hip),
which path kernel a batch of openings reaches from shapecases.path_kernel; each test states what it expects."""
import os
import subprocess
import sys

import numpy as np
import pytest

import soundcases as C
from helpers import soundness_driver as D
from helpers.forest import SENTINEL, _np, _tag, _torch
from testsupport import soundness as S
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT64 = np.uint64(SENTINEL & (2 ** 64 - 1))
TAIL = D.TAIL
LANE_GROUP_MAX = 8192  # kernels.h coop8: a batch of up to 8,192 runs on lane groups


def _outputs(n):
    """ok, roots out, digests, bad count: each with a canary tail"""
    import torch
    return (torch.full((n + TAIL,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((n + TAIL, 4), SENTINEL, dtype=torch.int64, device="cuda:0"),
            torch.full((1 + TAIL,), -1, dtype=torch.int64, device="cuda:0"), torch.zeros(1 + TAIL, dtype=torch.int32, device="cuda:0"))


def _intact(n, ok, roots, hashed, bad):
    return bool((ok[n:] == 7).all()) and bool((roots[n:] == SENTINEL).all()) and bool((hashed[1:] == -1).all()) and not bool(bad[1:].any())


def _root_or_none(r):
    return None if (r == SENT64).all() else r


def _same_root(got, want):
    return (got is None and want is None) or (got is not None and want is not None and np.array_equal(got, want))


# ---------------------------------------------------------------------------------------------- shared proof, one tree
def _shared_verify(ctx, arity, x):
    """one verification of the inputs x -> (ok, root_out or None where it was left alone, n_hashed, n_bad)"""
    ok, root, hashed, bad = _outputs(1)
    ctx.merkle_multiproof_verify_device(_tag(arity), x["n"], _torch(x["pos"].astype(np.uint32)), _torch(x["leaves"]), len(x["pos"]), _torch(x["buf"]),
                                        x["plen"], _torch(x["root"]), ok[:1], d_root_out=root[0], d_n_hashed=hashed[:1], d_n_bad=bad[:1], arity=arity)
    ctx.sync()
    assert _intact(1, ok, root, hashed, bad)
    return int(ok[0]), _root_or_none(_np(root[0])), int(hashed[0]), int(bad[0])


def _shared_sweep(ctx, arity, cases, verdicts, what):
    for (cls, x, _), want in zip(cases, verdicts):
        got = _shared_verify(ctx, arity, x)
        assert got[0] == want[0] and _same_root(got[1], want[1]) and got[2:] == want[2:], (what, cls, got, want)
    assert _shared_verify(ctx, arity, cases[0][1])[0] == 1  # the good proof, afterwards


@pytest.mark.parametrize("arity,n", [(a, n) for a in (4, 2) for n in C.SHARED_SHAPES[a]])
def test_every_change_to_a_shared_proof_of_one_tree(gpu_ctx, oracle_mod, arity, n):
    """every case of every class for every position set, one verify call each: ok, root_out (left alone where the structure fails),
    n_hashed and n_bad are the model's.  Every level's bound is far below 8,192: k_mp_digest_coop."""
    for name, _, cases, verdicts in C.shared_single(arity, n):
        _shared_sweep(gpu_ctx, arity, cases, verdicts, (arity, n, name))


@pytest.mark.parametrize("arity", [4, 2])
def test_proof_scalars_on_either_side_of_a_scan_tile_border(gpu_ctx, oracle_mod, arity):
    """every other leaf of 4^5 + 5 (2^10 + 1) leaves: three 256-element tiles at level 0 (arity 2: at level 1 as well); the flip, + p and
    swap of the proof scalars of the parents on either side of each border and of the proof's last scalar.  k_mp_digest_coop."""
    x, at, cases, verdicts = C.shared_tiles(arity)
    assert len(x["pos"]) > 2 * C.TILE and len(at) >= 3
    _shared_sweep(gpu_ctx, arity, cases, verdicts, ("tiles", arity))


# ---------------------------------------------------------------------------------------------- shared proof, a forest
def _forest_verify(ctx, arity, F):
    """one verification of the forest inputs F -> (ok (T,), [root_out or None], n_hashed, n_bad)"""
    T, k = len(F["sizes"]), len(F["tid"])
    ok, roots, hashed, bad = _outputs(T)
    call = ctx.merkle4_forest_ragged_multiproof_verify_device if arity == 4 else ctx.merkle2_forest_ragged_multiproof_verify_device
    call(_tag(arity), _torch(F["off"]), int(F["off"][-1]), T, int(F["sizes"].max()), _torch(F["tid"].astype(np.uint32)), _torch(F["lid"].astype(np.uint64)),
         _torch(F["leaves"]), k, _torch(F["proof"]) if len(F["proof"]) else None, F["plen"], _torch(F["po"]), _torch(F["roots"]), ok[:T],
         d_roots_out=roots[:T], d_n_hashed=hashed[:1], d_n_bad=bad[:1])
    ctx.sync()
    assert _intact(T, ok, roots, hashed, bad)
    return ok[:T].cpu().numpy(), [_root_or_none(r) for r in _np(roots[:T])], int(hashed[0]), int(bad[0])


def _digest_kernels(F, arity):
    """the digest kernels of a forest verification, from the level bounds of forest_multiproof.hip: min(k, n_leaves / A^l + n_trees)"""
    k, n, T = len(F["tid"]), int(F["off"][-1]), len(F["sizes"])
    bounds = [min(k, n // arity ** l + T) for l in range(1, int(TS.depth(min(int(F["sizes"].max()), n), arity)) + 1)]
    return {"k_mp_digest_coop" if b <= LANE_GROUP_MAX else "k_mp_digest" for b in bounds}


def _forest_check(ctx, arity, F, want, what):
    ok, roots, hashed, bad = _forest_verify(ctx, arity, F)
    wrong = np.nonzero(ok != want[0])[0]
    assert wrong.size == 0, (what, "verdicts differ from the model's at trees", wrong[:8], ok[wrong[:8]])
    assert all(_same_root(g, w) for g, w in zip(roots, want[1])), what
    assert (hashed, bad) == want[2:], (what, hashed, bad, want[2:])


@pytest.mark.parametrize("arity,n", [(a, n) for a in (4, 2) for n in C.COPIES_SHAPES[a]])
def test_one_forest_call_carries_every_change(gpu_ctx, oracle_mod, arity, n):
    """copies of one tree, copy i with case i (every position set in turn); a copy that lies about its proof length or its leaf count
    moves an offset of the forest, so an untouched copy stands behind it and takes the model's verdict too.  d_ok is the model's vector,
    roots_out per tree too (left alone where the structure fails), n_hashed counts every tree."""
    F, where, cases, want = C.shared_copies(arity, n)
    assert {c[0] for c in cases} >= set(S.SHARED_CLASSES) and _digest_kernels(F, arity) == {"k_mp_digest_coop"}
    _forest_check(gpu_ctx, arity, F, want, (arity, n))
    for i, (cls, _, expectation) in enumerate(cases):  # (the classes' own claims, as the CPU test shows them for the model)
        claim = S.expected_ok(expectation)
        assert claim is None or want[0][where[i]] == claim, cls
    good = S.forest_of([cases[0][1]] * 3)
    assert _forest_verify(gpu_ctx, arity, good)[0].tolist() == [1, 1, 1]


@pytest.mark.parametrize("every", [1, 3])
def test_a_random_change_in_the_trees_of_the_many_forest(gpu_ctx, oracle_mod, every):
    """3,000 trees of 16 .. 40 leaves, 12 pairs each: levels 1 and 2 are bounded above 8,192 records and run on the one-lane k_mp_digest,
    level 3 on k_mp_digest_coop.  One random case in every tree, then in every third tree only: the verdicts are exact"""
    F, classes, want = C.shared_many(every)
    assert _digest_kernels(F, 4) == {"k_mp_digest", "k_mp_digest_coop"}
    assert len({c for c in classes if c}) >= 8 and sum(c is not None for c in classes) == (C.MANY_TREES + every - 1) // every
    _forest_check(gpu_ctx, 4, F, want, ("many", every))
    assert _forest_verify(gpu_ctx, 4, S.forest_of(C.many_good()[:5]))[0].all()


# ---------------------------------------------------------------------------------------------- openings
def _child(jobs, env, tmp_path):
    """the sweeps `jobs` in ONE fresh process under `env` -> what run_sweep returns there for each"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **D.pack(jobs))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "soundness_driver.py"), src, dst], env=dict(os.environ, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(dst) as z:
        return D.unpack(z)


def _check_sweep(sw, got, what):
    wrong = np.nonzero(got["ok"] != sw["ok"])[0]
    assert wrong.size == 0, (what, "verdicts differ from the model's at rows", wrong[:8], sw["cls"][wrong[:8]], sw["rows"][wrong[:8]])
    for (cls, _, want), ok in zip(sw["roots"], got["alt"]):
        assert np.array_equal(ok, want) and not ok.any(), (what, cls)
    assert got["after"].all(), what


@pytest.mark.parametrize("arity", [4, 2])
def test_every_change_to_an_opening_of_fixed_depth_on_lane_groups(gpu_ctx, oracle_mod, arity):
    """every case of every leaf's opening of each tree in one batch (p252_merkle{4,2}_verify_batch_device has one root per call, so one
    batch per tree), in calls of at most 8,192 rows: k_merkle4_path_coop (arity 2: k_merkle2_path at every size)"""
    for depth, n in C.FIXED_TREES[arity]:
        sw = C.fixed_openings(arity, depth, n)
        got = D.run_sweep(gpu_ctx, D.job(sw, arity, True, chunk=LANE_GROUP_MAX))
        assert got["kernel"] == ("k_merkle4_path_coop" if arity == 4 else "k_merkle2_path")
        _check_sweep(sw, got, (arity, depth, n))


def test_every_change_to_an_opening_of_fixed_depth_on_one_lane(oracle_mod, tmp_path):
    """the same batches whole, in one child process with P252_COOP_MAX_NODES=0: depth 3 on k_merkle4_path, depth 4 (buffers as allocated:
    aligned) on the line-fetching k_merkle4_path_lines, arity 2 on k_merkle2_path"""
    trees = [(arity, depth, n) for arity in (4, 2) for depth, n in C.FIXED_TREES[arity]]
    sweeps = [C.fixed_openings(*t) for t in trees]
    for (arity, depth, n), sw, got in zip(trees, sweeps, _child([D.job(sw, t[0], True) for t, sw in zip(trees, sweeps)], {"P252_COOP_MAX_NODES": "0"}, tmp_path)):
        assert str(got["kernel"]) == ("k_merkle2_path" if arity == 2 else "k_merkle4_path_lines" if depth == 4 else "k_merkle4_path")
        _check_sweep(sw, got, (arity, depth, n))


def test_every_change_to_an_opening_of_depth_4_without_the_line_fetch(oracle_mod, tmp_path):
    """depth 4 on the one-lane k_merkle4_path: a child process with P252_COOP_MAX_NODES=0 and P252_LINE_FETCH=0"""
    sweeps = [C.fixed_openings(4, 4, n) for n in (4 ** 4, 65)]
    for sw, got in zip(sweeps, _child([D.job(sw, 4, True) for sw in sweeps], {"P252_COOP_MAX_NODES": "0", "P252_LINE_FETCH": "0"}, tmp_path)):
        assert str(got["kernel"]) == "k_merkle4_path"
        _check_sweep(sw, got, "depth 4 without the line fetch")


@pytest.mark.parametrize("arity", [4, 2])
def test_every_change_to_a_ragged_opening(gpu_ctx, oracle_mod, arity):
    """every leaf of the trees of helpers.forest._mix in ONE batch with the depth byte, the tree id and the rows past the depth, sorted
    by depth on the device (k_path_ragged, k_compare_roots_gather)"""
    sw = C.ragged_openings(arity)
    got = D.run_sweep(gpu_ctx, D.job(sw, arity, False))
    assert got["sorted"] == 1
    _check_sweep(sw, got, ("ragged", arity))


def test_every_change_to_a_ragged_opening_without_the_depth_sort(gpu_ctx, oracle_mod, tmp_path):
    """the same batches in a child process with P252_RAGGED_SORT=0: the verdict vectors of this process, which sorts"""
    sweeps = [C.ragged_openings(arity) for arity in (4, 2)]
    jobs = [D.job(sw, arity, False) for sw, arity in zip(sweeps, (4, 2))]
    for sw, J, plain in zip(sweeps, jobs, _child(jobs, {"P252_RAGGED_SORT": "0"}, tmp_path)):
        assert int(plain["sorted"]) == 0 and np.array_equal(plain["ok"], D.run_sweep(gpu_ctx, J)["ok"])
        _check_sweep(sw, plain, "ragged, unsorted")


@pytest.mark.parametrize("arity", [4, 2])
def test_every_change_to_an_anchored_opening(gpu_ctx, oracle_mod, arity):
    """the trees of test_forest_anchor_gpu's small forest as they were one leaf earlier and at half their leaves: the device's anchor roots
    (roots of a partial old tree: another code path than the build's) and anchored openings are the oracle's for the first c leaves, and
    the ragged sweep on them, against the device's anchor roots, gives the model's verdicts"""
    import torch
    from poseidon252_amd import merkle
    sizes, trees, a_tree, a_count, o_anchor, o_leaf = C.anchor_forest(arity)
    d, d_off = _torch(np.concatenate(trees)), _torch(TS.offsets(sizes))
    roots, d_lv = torch.zeros((len(sizes), 4), dtype=torch.int64, device="cuda:0"), torch.zeros((TS.levels_bound(sum(sizes), len(sizes), max(sizes), arity), 4),
                                                                                               dtype=torch.int64, device="cuda:0")
    gpu_ctx.merkle_forest_ragged_device(_tag(arity), d, d_off, len(sizes), max(sizes), roots, d_lv, None, arity=arity)
    a_roots, a_depths, (lv, sib, pos, dep, stride), (bad_anchors, bad), _ = merkle.forest_ragged_anchor_openings(
        gpu_ctx, _tag(arity), d, d_off, len(sizes), max(sizes), d_lv, a_tree, a_count, o_anchor, o_leaf, arity=arity)
    torch.cuda.synchronize()
    sw = C.anchored_openings(arity)
    good = sw["good"]
    assert int(bad_anchors) == 0 and int(bad) == 0 and stride == good["stride"]
    assert np.array_equal(_np(a_roots), good["roots"]) and np.array_equal(o_anchor, good["tid"])
    for name, t in (("leaves", lv), ("sib", sib), ("pos", pos), ("dep", dep)):
        assert np.array_equal(_np(t).reshape(good[name].shape), good[name]), name
    J = D.job(sw, arity, False)
    J["roots"] = _np(a_roots)
    _check_sweep(sw, D.run_sweep(gpu_ctx, J), ("anchored", arity))
