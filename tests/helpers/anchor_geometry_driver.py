"""Driver of the launch-geometry test of tests/test_forest_anchor_gpu.py — runs it in this process (imported) or in one of its own:

  python tests/helpers/anchor_geometry_driver.py

for the child that sets P252_COOP_MAX_NODES=0, which the library reads once per process: the anchors' digests then run the one-lane
build where the default environment runs the lane-group build.  One tree of A^5 + 3 leaves per arity; m anchors at random counts and k
openings of random leaves below their anchor's count, for every m in M and k in K.  Every opening must pass
p252_merkle{4,2}_forest_ragged_verify_device against the anchor roots; every anchor root must be d_old_roots_out of consistency
extraction plus verification of the same (tree, count) where the count is below n_t, and the forest's root where it is n_t; the digest
count must be the model's whatever k is.  A mismatch raises.  Prints a JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from testsupport import forestanchor as FA  # noqa: E402
from testsupport import treeshape as TS  # noqa: E402
from helpers.forest import Old, _np, _tag, _torch  # noqa: E402

M = (1, 7, 8, 9, 63, 64, 65, 257)
K = (1, 255, 256, 257, 5000)


def run(ctx, arity, seed=0xA90):
    """-> {"calls", "openings", "digests"}; raises on the first mismatch"""
    import torch
    from poseidon252_amd import merkle
    rng = np.random.default_rng(seed + arity)
    n = arity ** 5 + 3
    flat = rng.integers(0, 1 << 60, (n, 4)).astype(np.uint64)
    f = Old(ctx, arity, flat, np.array([0, n], dtype=np.uint64), n)
    D = int(TS.depth(n, arity))
    tag = _tag(arity)
    extract = ctx.merkle4_forest_ragged_consistency_device if arity == 4 else ctx.merkle2_forest_ragged_consistency_device
    verify = ctx.merkle4_forest_consistency_verify_device if arity == 4 else ctx.merkle2_forest_consistency_verify_device
    calls = openings = digests = 0
    for m in M:
        counts = rng.integers(1, n + 1, m)
        counts[0] = n if m > 1 else arity ** 5 + 1  # the whole tree among them
        if m > 2:
            counts[1], counts[2] = arity ** 5, arity ** 3 + arity  # a power of the arity, trailing zero digits
        want_hashed = sum(FA.old_digests(int(c), arity) for c in counts)
        # the other route to the roots: consistency extraction plus verification of the same (tree, count)
        grown = counts < n
        d_tid, d_old = torch.zeros(m, dtype=torch.int32, device="cuda:0"), _torch(counts.astype(np.uint64))
        newc = torch.zeros(m, dtype=torch.int64, device="cuda:0")
        p_lv, p_sib = torch.zeros((m, 4), dtype=torch.int64, device="cuda:0"), torch.zeros((m, D, arity - 1, 4), dtype=torch.int64, device="cuda:0")
        p_pos, p_dep = torch.zeros((m, D), dtype=torch.uint8, device="cuda:0"), torch.zeros(m, dtype=torch.uint8, device="cuda:0")
        ok = torch.zeros(m, dtype=torch.uint8, device="cuda:0")
        old_out = torch.zeros((m, 4), dtype=torch.int64, device="cuda:0")
        new_roots = f.roots[:1].expand(m, 4).contiguous()
        extract(f.d, f.d_off, 1, n, f.d_lv, d_tid, d_old, m, newc, p_lv, p_sib, p_pos, p_dep, None)
        verify(tag, d_old, new_roots, newc, new_roots, p_lv, p_sib, p_pos, p_dep, D, m, ok, None, 0, old_out, None, None)
        torch.cuda.synchronize()
        want_roots = np.where(grown[:, None], _np(old_out), _np(f.roots)[:1])
        hashed_by_k = []
        for k in K:
            o_anchor = rng.integers(0, m, k)
            o_leaf = (rng.random(k) * counts[o_anchor]).astype(np.int64)
            o_leaf[0] = counts[o_anchor[0]] - 1  # the last leaf below the count
            roots, depths, op, (bad_anchors, bad), hashed = merkle.forest_ragged_anchor_openings(ctx, tag, f.d, f.d_off, 1, n, f.d_lv, np.zeros(m, np.int64),
                                                                                               counts, o_anchor, o_leaf, arity=arity)
            d_ok = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
            ctx.merkle_forest_ragged_verify_device(tag, *op, _torch(o_anchor.astype(np.uint32)), roots, m, d_ok, k, arity=arity)
            torch.cuda.synchronize()
            where = (arity, m, k)
            assert int(bad_anchors) == 0 and int(bad) == 0, where
            assert np.array_equal(_np(roots), want_roots), (where, np.nonzero((_np(roots) != want_roots).any(axis=1))[0][:8], counts[:8])
            assert np.array_equal(depths.cpu().numpy(), TS.depth(counts, arity).astype(np.uint8)), where
            assert np.array_equal(op[3].cpu().numpy(), TS.depth(counts[o_anchor], arity).astype(np.uint8)), where
            assert np.array_equal(_np(op[0]), flat[o_leaf]), where
            assert bool(d_ok.all()), (where, torch.nonzero(d_ok == 0)[:8].flatten().tolist())
            hashed_by_k.append(int(hashed))
            calls, openings = calls + 1, openings + k
        assert hashed_by_k == [want_hashed] * len(K), (arity, m, hashed_by_k, want_hashed)
        digests += want_hashed
    return {"calls": calls, "openings": openings, "digests": digests}


def main():
    import poseidon252_amd as P
    ctx = P.Context(0)
    report = {str(arity): run(ctx, arity) for arity in (4, 2)}
    print(json.dumps({"anchor_geometry": "ok", "coop_max_nodes": os.environ.get("P252_COOP_MAX_NODES"), "arities": report}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
