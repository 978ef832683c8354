"""Every family of `_device` calls that works in the context's per-stream scratch pair (csrc/api_util.hpp with_stream_scratch, behind the entry points of csrc/api.cpp and csrc/api_forest.cpp), mixed on
six streams of ONE context: the context keeps four pairs, so the fifth and sixth stream take a pair over behind its event, and with
the assignment rotated each round every pair is taken over by a family that asks other sizes of it.  Each output must equal that of
the same call made alone on the default stream."""
import numpy as np
import pytest

from helpers.forest import _tag, _torch
from testsupport import treeshape as TS
from testsupport.device import tree_device  # (p252_merkle{4,2}_tree_device on the current stream)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 17, 64, 65, 300]
K = 50


def _families(ctx, oracle, arity):
    """six (name, outputs(), call(outputs)) triples; call() enqueues on torch's current stream and writes only into `outputs`"""
    import torch
    from poseidon252_amd import hash as H
    from poseidon252_amd import levels_len
    dev, tag = torch.device("cuda:0"), _tag(arity)
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    rng = np.random.default_rng(40 + arity)
    # the forest, built once with its levels: one copy that is only read, one that the update family rewrites (the same k updates
    # every time, so each run leaves the same leaves, levels and roots)
    n_trees, max_leaves, n_leaves, D = len(SIZES), max(SIZES), sum(SIZES), TS.depth(max(SIZES), arity)
    d_fl, d_off = _torch(oracle.fill_random(0x71, n_leaves)), _torch(TS.offsets(SIZES))
    d_froots, d_flv = i64(n_trees, 4), i64(TS.levels_bound(n_leaves, n_trees, max_leaves, arity) + 1, 4)
    ctx.merkle_forest_ragged_device(tag, d_fl, d_off, n_trees, max_leaves, d_froots, d_flv, arity=arity)
    d_ul, d_ulv = d_fl.clone(), d_flv.clone()
    pairs = rng.permutation(n_leaves)[:K]  # distinct (tree, leaf) pairs
    tid = np.searchsorted(np.cumsum(SIZES), pairs, side="right")
    lid = pairs - TS.offsets(SIZES)[tid].astype(np.int64)
    d_tid, d_lid, d_new = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64)), _torch(oracle.fill_random(0x72, K))
    # the stored tree of the shared proof
    n_mp, k_mp = 1000, 37
    d_ml, d_mroot, d_mlv = _torch(oracle.fill_random(0x73, n_mp)), i64(4), i64(levels_len(n_mp, arity), 4)
    tree_device(ctx, arity, tag, d_ml, n_mp, d_mroot, d_mlv)
    d_midx = _torch(np.sort(rng.permutation(n_mp)[:k_mp]).astype(np.uint32))
    bound = ctx.merkle_multiproof_bound(n_mp, k_mp, arity=arity)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.merkle_multiproof_device(d_ml, n_mp, d_mlv, d_midx, k_mp, i64(k_mp, 4), i64(bound, 4), d_len, arity=arity)
    proof_len = int(d_len)  # (the verify call takes it from the host)
    assert 0 < proof_len <= bound
    # the root-only tree and the messages of different lengths
    n_tree = 4 ** 6 + 3
    d_tl = _torch(oracle.fill_random(0x74, n_tree))
    lens = 1 + np.arange(200) % 40
    d_msg, d_moff = _torch(oracle.fill_random(0x75, int(lens.sum()))), _torch(TS.offsets(lens))
    d_tags = _torch(H.ragged_tags(H.Domain.Other, 1, 40))

    def tree(o):
        tree_device(ctx, arity, tag, d_tl, n_tree, o[0], None)

    def forest(o):
        ctx.merkle_forest_ragged_device(tag, d_fl, d_off, n_trees, max_leaves, o[0], None, arity=arity)

    def open_verify(o):
        ctx.merkle_forest_ragged_openings_device(d_fl, d_off, n_trees, max_leaves, d_flv, d_tid, d_lid, K, out=o[:4], arity=arity)
        ctx.merkle_forest_ragged_verify_device(tag, o[0], o[1], o[2], o[3], D, d_tid, d_froots, n_trees, o[4], K, arity=arity)

    def update(o):
        ctx.merkle_forest_ragged_update_device(tag, d_ul, d_off, n_trees, max_leaves, d_ulv, d_tid, d_lid, d_new, K, d_roots=o[0], arity=arity)

    def ragged(o):
        ctx.hash_ragged_device(d_tags, 40, d_msg, d_moff, 1, o[0], 200)

    def multiproof(o):
        ctx.merkle_multiproof_device(d_ml, n_mp, d_mlv, d_midx, k_mp, o[0], o[1], o[2], arity=arity)
        ctx.merkle_multiproof_verify_device(tag, n_mp, d_midx, o[0], k_mp, o[1], proof_len, d_mroot, o[3], d_root_out=o[4], arity=arity)

    return [("tree", lambda: [i64(4)], tree),
            ("forest", lambda: [i64(n_trees, 4)], forest),
            ("openings+verify", lambda: [i64(K, 4), i64(K, D, arity - 1, 4), u8(K, D), u8(K), u8(K)], open_verify),
            ("update", lambda: [i64(n_trees, 4)], update),
            ("hash_ragged", lambda: [i64(200, 1, 4)], ragged),
            ("multiproof+verify", lambda: [i64(k_mp, 4), i64(bound, 4), torch.zeros(1, dtype=torch.int64, device=dev), u8(1), i64(4)], multiproof)], (d_ul, d_ulv)


@pytest.mark.parametrize("arity", [4, 2])
def test_six_families_on_six_streams_of_one_context(gpu_ctx, oracle_mod, arity):
    import torch
    families, updated = _families(gpu_ctx, oracle_mod, arity)
    alone = []
    for _, outputs, call in families:  # each call alone, on the default stream
        o = outputs()
        call(o)
        torch.cuda.synchronize()
        alone.append([t.clone() for t in o])
    assert bool(alone[2][4].all()) and int(alone[5][3]) == 1, "a verify refuses what was just extracted"
    assert not bool((alone[0][0] == 0).all()) and int(alone[5][2]) > 0
    state = [t.clone() for t in updated]  # the updated forest after its first update
    streams = [torch.cuda.Stream() for _ in families]
    outs = [[outputs() for _, outputs, _ in families] for _ in range(3)]
    torch.cuda.synchronize()
    for rnd in range(3):
        for f, (_, _, call) in enumerate(families):
            with torch.cuda.stream(streams[(f + rnd) % len(streams)]):
                call(outs[rnd][f])
    torch.cuda.synchronize()
    for rnd in range(3):
        for f, (name, _, _) in enumerate(families):
            for i, (got, exp) in enumerate(zip(outs[rnd][f], alone[f])):
                assert torch.equal(got, exp), (name, "round %d" % rnd, "output %d" % i)
    assert all(torch.equal(a, b) for a, b in zip(updated, state)), "the updated forest changed under the same updates"
