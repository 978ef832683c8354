"""Many leaves of ONE stored tree behind one shared proof (p252_merkle{4,2}_multiproof_device / _verify_device; csrc/multiproof.hip)
on the GPU: the proof's bytes and length, the leaves, the recomputed root and the digest count against the numpy model of the format
(testsupport/multiproofmodel.py), the roots against the oracle, k = 1 against the per-leaf openings, shapes that leave one scan tile
and the 8-lane digest, rejected proofs, bad positions, a short proof buffer, streams, p252_trim and a forest's tree block."""
import numpy as np
import pytest

from helpers.forest import SENTINEL, _build, _np, _single_extract as _extract, _single_verify as _verify, _tag, _torch
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport.device import tree_device
from testsupport.multiproofmodel import multiproof_counts, multiproof_extract  # (the numpy model; tests/test_multiproof_cpu.py checks it)
from testsupport.soundness import index_sets as _index_sets  # (the position sets: the soundness sweep's too)
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

_TREES = {}


def _leaves(n, seed):
    """n scalars below 2^252 (every limb below 2^60)"""
    return np.random.default_rng(seed).integers(0, 1 << 60, size=(n, 4), dtype=np.uint64)


def _tree(ctx, arity, n):
    """one stored tree per (arity, n), built once -> (leaves, levels, root) on the host and (d, d_lv, d_root) on the device"""
    import torch
    from poseidon252_amd import levels_len
    if (arity, n) not in _TREES:
        leaves = _leaves(n, 1000 * arity + n % 997)
        d = _torch(leaves)
        d_root = torch.empty(4, dtype=torch.int64, device=d.device)
        d_lv = torch.empty((max(levels_len(n, arity), 1), 4), dtype=torch.int64, device=d.device)
        tree_device(ctx, arity, _tag(arity), d, n, d_root, d_lv if n > 1 else None)
        torch.cuda.synchronize()
        _TREES[(arity, n)] = (leaves, _np(d_lv)[:levels_len(n, arity)], _np(d_root), d, d_lv, d_root)
    return _TREES[(arity, n)]


def _round_trip(ctx, arity, n, pos):
    """extract + verify of sorted distinct `pos`, everything compared with the model and the tree's root"""
    leaves, levels, root, d, d_lv, _ = _tree(ctx, arity, n)
    pos = np.asarray(pos, dtype=np.int64)
    want = multiproof_extract(leaves, levels, pos, arity)
    want_len, want_hashed = multiproof_counts(n, pos, arity)
    assert want.shape[0] == want_len <= ctx.merkle_multiproof_bound(n, len(pos), arity)
    out, proof, plen, bad = _extract(ctx, arity, n, d, d_lv, pos)
    print("arity %d n %d k %d: proof_len %d (model %d), bad %d" % (arity, n, len(pos), plen, want_len, bad))
    assert (plen, bad) == (want_len, 0)
    assert np.array_equal(proof[:plen], want) and np.array_equal(out, leaves[pos])
    ok, root_out, hashed, bad = _verify(ctx, arity, n, pos, out, proof[:plen], plen, root)
    print("  verify: ok %d, n_hashed %d (model %d), bad %d" % (ok, hashed, want_hashed, bad))
    assert (ok, hashed, bad) == (1, want_hashed, 0)
    assert root_out is not None and np.array_equal(root_out, root)
    return out, proof[:plen]


SHAPES = [(4, n) for n in (1, 2, 4, 5, 16, 17, 21, 64, 1000)] + [(2, n) for n in (1, 2, 3, 7, 33, 1000)]


@pytest.mark.parametrize("arity,n", SHAPES)
def test_proof_and_verification_match_the_model(gpu_ctx, oracle_mod, arity, n):
    leaves, _, root, _, _, _ = _tree(gpu_ctx, arity, n)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    assert np.array_equal(root, tree(_tag(arity), leaves)[0])  # (n <= 1000: the tree's root is the oracle's)
    for name, pos in _index_sets(n, arity).items():
        _, proof = _round_trip(gpu_ctx, arity, n, pos)
        if name == "all" or n == 1:
            assert proof.shape[0] == 0


@pytest.mark.parametrize("arity,n", [(4, 64), (4, 21), (4, 1000), (2, 32), (2, 33)])
def test_one_leaf_is_the_per_leaf_opening_without_the_padding(gpu_ctx, arity, n):
    import torch
    leaves, _, _, d, d_lv, _ = _tree(gpu_ctx, arity, n)
    picks = sorted({0, 1, n // 2, n - 2, n - 1})
    o_l, o_s, o_p, depth = gpu_ctx.merkle4_openings_device(d, n, d_lv, _torch(np.asarray(picks, np.uint32)), len(picks), check=True, arity=arity)
    torch.cuda.synchronize()
    sib = _np(o_s).reshape(len(picks), depth, arity - 1, 4)
    for row, i in enumerate(picks):
        keep, node, w = [], i, n
        for l in range(depth):  # the sibling slots of the opening, ascending, without those at or past the level's width
            base = node - node % arity
            others = [base + j for j in range(arity) if base + j != node]
            keep += [sib[row, l, s] for s, c in enumerate(others) if c < w]
            node, w = node // arity, (w + arity - 1) // arity
        out, proof, plen, bad = _extract(gpu_ctx, arity, n, d, d_lv, [i])
        assert bad == 0 and plen == len(keep) and np.array_equal(proof[:plen], np.array(keep, dtype=np.uint64).reshape(-1, 4))
        assert np.array_equal(out[0], leaves[i]) and np.array_equal(out[0], _np(o_l)[row])
        if n in (64, 32):  # a complete tree: nothing dropped, and the bound is reached
            assert plen == depth * (arity - 1) == gpu_ctx.merkle_multiproof_bound(n, 1, arity)


@pytest.mark.parametrize("arity,n,what", [(4, 4 ** 7 + 5, "random 5000"), (4, 4 ** 7 + 5, "run"), (4, 4 ** 8 + 1, "random 40000"),
                                          (2, 2 ** 16 + 1, "random 40000")])
def test_more_than_one_scan_tile_and_both_digest_kernels(gpu_ctx, arity, n, what):
    """5,000 positions: 20 scan tiles at level 0, every digest level on the 8-lane kernel; 40,000: level 1 has more than 8,192 nodes
    and takes the one-lane kernel; the run [3, 3003): whole parents, whose runs cross tile borders"""
    if what == "run":
        pos = np.arange(3, 3003)
    else:
        pos = np.sort(np.random.default_rng(5).choice(n, int(what.split()[1]), replace=False))
    if what == "random 40000":
        from testsupport.multiproofmodel import multiproof_model
        assert multiproof_model(n, pos, arity)[1][1].size > 8192
    _round_trip(gpu_ctx, arity, n, pos)


@pytest.mark.parametrize("arity", [4, 2])
def test_a_changed_proof_leaf_length_or_root_is_rejected(gpu_ctx, arity):
    n = 1000
    leaves, levels, root, d, d_lv, _ = _tree(gpu_ctx, arity, n)
    pos = np.sort(np.random.default_rng(6).choice(n, 100, replace=False))
    out, proof = _round_trip(gpu_ctx, arity, n, pos)
    plen = proof.shape[0]
    assert plen > 2
    spare = np.concatenate([proof, proof[:1]])
    for at in (0, plen // 2, plen - 1):  # one proof scalar changed (one bit of one limb)
        changed = proof.copy()
        changed[at, 1] ^= np.uint64(1)
        assert _verify(gpu_ctx, arity, n, pos, out, changed, plen, root)[0] == 0
    for at in (0, 57, 99):  # one leaf changed
        changed = out.copy()
        changed[at, 0] ^= np.uint64(1 << 17)
        assert _verify(gpu_ctx, arity, n, pos, changed, proof, plen, root)[0] == 0
    ok, root_out, _, _ = _verify(gpu_ctx, arity, n, pos, out, proof, plen - 1, root)  # one scalar short
    assert ok == 0 and root_out is None
    ok, root_out, _, _ = _verify(gpu_ctx, arity, n, pos, out, spare, plen + 1, root)  # one scalar long, the spare scalar in the buffer
    assert ok == 0 and root_out is None
    wrong = root.copy()
    wrong[3] ^= np.uint64(1)
    ok, root_out, _, _ = _verify(gpu_ctx, arity, n, pos, out, proof, plen, wrong)  # the proof is whole, the root another
    assert ok == 0 and np.array_equal(root_out, root)
    assert _verify(gpu_ctx, arity, n, pos, out, proof, plen, root)[0] == 1
    # the same leaves under other positions: another structure
    moved = pos.copy()
    moved[-1] = pos[-1] + 1 if pos[-1] + 1 < n else pos[-1] - 1 if pos[-1] - 1 > pos[-2] else pos[-1]
    if moved[-1] != pos[-1]:
        assert _verify(gpu_ctx, arity, n, moved, out, proof, plen, root)[0] == 0


@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("name,pos,n_bad", [("unsorted", [5, 3, 9], 1), ("duplicate", [3, 3, 9], 1), ("outside", [3, 9, 1000], 1),
                                            ("far outside", [3, 9, 0xFFFFFFFF], 1), ("descending", [9, 8, 7, 6], 3),
                                            ("outside twice", [2000, 3000], 2), ("outside then below", [1000, 4], 2)])
def test_bad_positions_are_counted_and_refused(gpu_ctx, arity, name, pos, n_bad):
    n = 1000
    leaves, _, root, d, d_lv, _ = _tree(gpu_ctx, arity, n)
    _, _, plen, bad = _extract(gpu_ctx, arity, n, d, d_lv, pos)  # (_extract ends in p252_sync: no error)
    assert (plen, bad) == (0, n_bad), name
    some = leaves[:len(pos)]
    for proof_len in (0, 3):
        ok, root_out, hashed, bad = _verify(gpu_ctx, arity, n, pos, some, leaves[:proof_len], proof_len, root)
        assert (ok, root_out, hashed, bad) == (0, None, 0, n_bad), name
    # more positions than leaves cannot be strictly ascending
    tiny = _tree(gpu_ctx, arity, 2)
    _, _, plen, bad = _extract(gpu_ctx, arity, 2, tiny[3], tiny[4], [0, 1, 1])
    assert (plen, bad) == (0, 1)
    # and the context is in order
    _round_trip(gpu_ctx, arity, n, [3, 9])


@pytest.mark.parametrize("arity", [4, 2])
def test_a_short_proof_buffer_reports_the_need_and_is_not_overrun(gpu_ctx, arity):
    n = 4 ** 7 + 5
    leaves, levels, _, d, d_lv, _ = _tree(gpu_ctx, arity, n)
    pos = np.sort(np.random.default_rng(8).choice(n, 700, replace=False))
    want = multiproof_extract(leaves, levels, pos, arity)
    sentinel = np.uint64(SENTINEL & (2 ** 64 - 1))
    for cap in (0, 1, want.shape[0] // 2, want.shape[0] - 1, want.shape[0]):
        out, proof, plen, bad = _extract(gpu_ctx, arity, n, d, d_lv, pos, cap=cap, pad=5)
        assert (plen, bad) == (want.shape[0], 0)
        assert np.array_equal(proof[:cap], want[:cap]) and (proof[cap:] == sentinel).all()
        assert np.array_equal(out[:len(pos)], leaves[pos]) and (out[len(pos):] == sentinel).all()


def test_null_arguments_and_empty_batches_are_refused(gpu_ctx):
    import torch
    leaves, _, root, d, d_lv, d_root = _tree(gpu_ctx, 4, 64)
    idx = torch.zeros(4, dtype=torch.int32, device=d.device)
    out = torch.zeros((4, 4), dtype=torch.int64, device=d.device)
    plen = torch.zeros(1, dtype=torch.int64, device=d.device)
    ok = torch.zeros(1, dtype=torch.uint8, device=d.device)
    with pytest.raises(ValueError):
        gpu_ctx.merkle_multiproof_device(d, 64, d_lv, idx, 0, out, None, plen)  # k == 0
    with pytest.raises(ValueError):
        gpu_ctx.merkle_multiproof_device(d, 0, None, idx, 1, out, None, plen)  # n_leaves == 0
    with pytest.raises(ValueError):
        gpu_ctx.merkle_multiproof_verify_device(_tag(4), 64, idx, out, 0, None, 0, d_root, ok)
    with pytest.raises(ValueError):
        gpu_ctx.merkle_multiproof_verify_device(_tag(4), 0, idx, out, 1, None, 0, d_root, ok)
    assert gpu_ctx.merkle_multiproof_bound(0, 3) == 0 and gpu_ctx.merkle_multiproof_bound(1, 1) == 0
    assert gpu_ctx.merkle_multiproof_bound(64, 64) == 0 and gpu_ctx.merkle_multiproof_bound(64, 1, arity=2) == 6


@pytest.mark.parametrize("arity", [4, 2])
def test_another_stream_and_a_trimmed_context_give_the_same(gpu_ctx, arity):
    import torch
    n = 4 ** 7 + 5
    pos = np.sort(np.random.default_rng(9).choice(n, 3000, replace=False))
    first = _round_trip(gpu_ctx, arity, n, pos)
    with torch.cuda.stream(torch.cuda.Stream()):
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
        second = _round_trip(gpu_ctx, arity, n, pos)
    torch.cuda.synchronize()
    gpu_ctx.trim()
    assert gpu_ctx.scratch_residue() == 0
    third = _round_trip(gpu_ctx, arity, n, pos)
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])


@pytest.mark.parametrize("arity", [4, 2])
def test_a_tree_block_of_a_ragged_forest_is_a_single_tree(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import levels_len
    sizes = [5, 300, 1, 17, 66]
    off = TS.offsets(sizes).astype(np.int64)
    lo = np.concatenate([[0], np.cumsum([levels_len(s, arity) for s in sizes])])
    flat = _leaves(sum(sizes), 77)
    d = _torch(flat)
    roots, d_lv = _build(gpu_ctx, arity, d, _torch(off.astype(np.uint64)), len(sizes), max(sizes))
    torch.cuda.synchronize()
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    for t, n in enumerate(sizes):
        blk, lv = d[off[t]:off[t + 1]], d_lv[lo[t]:lo[t + 1]]
        pos = np.arange(0, n, 3)
        want = multiproof_extract(flat[off[t]:off[t + 1]], _np(lv), pos, arity)
        out, proof, plen, bad = _extract(gpu_ctx, arity, n, blk, lv, pos)
        assert (plen, bad) == (want.shape[0], 0) and np.array_equal(proof[:plen], want)
        root = tree(_tag(arity), flat[off[t]:off[t + 1]])[0]
        assert np.array_equal(_np(roots)[t], root)
        ok, root_out, hashed, _ = _verify(gpu_ctx, arity, n, pos, out, proof[:plen], plen, root)
        assert ok == 1 and np.array_equal(root_out, root) and hashed == multiproof_counts(n, pos, arity)[1]


@pytest.mark.parametrize("arity", [4, 2])
def test_the_convenience_calls_sort_and_de_duplicate(gpu_ctx, arity):
    import poseidon252_amd as P
    n = 1000
    leaves, levels, root, d, d_lv, d_root = _tree(gpu_ctx, arity, n)
    idx, out, proof = P.merkle_multiproof(d, d_lv, [9, 3, 999, 3, 10], arity=arity, ctx=gpu_ctx)
    assert idx.cpu().tolist() == [3, 9, 10, 999]
    assert np.array_equal(_np(proof), multiproof_extract(leaves, levels, [3, 9, 10, 999], arity)) and np.array_equal(_np(out), leaves[[3, 9, 10, 999]])
    assert P.merkle_multiproof_verify(n, idx, out, proof, d_root, arity=arity, ctx=gpu_ctx) is True
    assert P.merkle_multiproof_verify(n, idx, out, proof[:-1], d_root, arity=arity, ctx=gpu_ctx) is False
    with pytest.raises(ValueError, match="outside"):
        P.merkle_multiproof(d, d_lv, [3, 1000], arity=arity, ctx=gpu_ctx)


def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_multiproof_api", tmp_path))
