"""The device helpers of the ragged-forest tests (build, openings, update, append, resize, journal, multiproof, the forest walk):
one definition of each, on the GPU through the Python binding.  The child processes that the GPU tests start import this module too."""
import time

import numpy as np

from testsupport import treeshape as TS
from testsupport.forestappend import model_leaves
# (the numpy model of what one update may hash; tests/test_forest_update_cpu.py checks it)
from testsupport.forestupdate import dirty_nodes as dirty_count  # noqa: F401

SENTINEL = -0x0123456789ABCDEF  # no scalar and no root has these limbs (the top limb is above the modulus')


def _mix(arity):  # tree sizes around every power of the arity that matters, and one tree a level deeper than the rest
    a = arity
    return [1, 2, 3, a, a + 1, a * a - 1, a * a, a * a + 1, 63, 65, (4 ** 5 + 1) if a == 4 else (2 ** 10 + 1)]


def _tag(arity):
    from poseidon252_amd import merkle as M
    return M.merkle4_tag() if arity == 4 else M.merkle2_tag()


def _torch(a, dev="cuda:0"):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _build(ctx, arity, d_leaves, d_off, n_trees, max_leaves):
    """the forest with its tree-major levels -> (roots, levels)"""
    import torch
    n_leaves = d_leaves.numel() // 4
    roots = torch.full((n_trees, 4), -1, dtype=torch.int64, device=d_leaves.device)
    d_lv = torch.zeros((max(TS.levels_bound(n_leaves, n_trees, max_leaves, arity), 1), 4), dtype=torch.int64, device=d_leaves.device)
    ctx.merkle_forest_ragged_device(_tag(arity), d_leaves, d_off, n_trees, max_leaves, roots, d_lv, None, arity=arity)
    return roots, d_lv


def _open(ctx, arity, d_leaves, d_off, n_trees, max_leaves, d_lv, tree_ids, leaf_ids):
    """openings, re-hash and verify of (tree_ids, leaf_ids) (numpy) -> dict of numpy results"""
    import torch
    k = len(tree_ids)
    d_tid, d_lid = _torch(np.asarray(tree_ids, np.uint32)), _torch(np.asarray(leaf_ids, np.uint64))
    bad = torch.zeros(2, dtype=torch.int32, device=d_leaves.device)
    lv, sib, pos, dep, D = ctx.merkle_forest_ragged_openings_device(d_leaves, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, k,
                                                                    d_n_bad=bad[:1], arity=arity)
    back = torch.full((k, 4), -1, dtype=torch.int64, device=d_leaves.device)
    ctx.merkle_path_ragged_device(_tag(arity), lv, sib, pos, dep, D, back, k, d_n_bad=bad[1:], arity=arity)
    return dict(leaves=lv, sib=sib, pos=pos, dep=dep, D=D, back=back, bad=bad, d_tid=d_tid, d_lid=d_lid)


def _verify(ctx, arity, o, d_roots, n_trees):
    import torch
    k = o["dep"].numel()
    ok = torch.full((k,), 7, dtype=torch.uint8, device=o["dep"].device)
    ctx.merkle_forest_ragged_verify_device(_tag(arity), o["leaves"], o["sib"], o["pos"], o["dep"], o["D"], o["d_tid"], d_roots, n_trees, ok, k,
                                           arity=arity)
    return ok


def _tree(oracle_mod, arity):
    return oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree


def _forest(ctx, arity, flat, off, max_leaves=None, tail=9):
    """the forest on the device, built into a sentinel-filled d_levels with `tail` scalars past the bound -> (d, d_off, roots, d_lv)"""
    import torch
    sizes = np.diff(off.astype(np.int64))
    n_trees = len(sizes)
    max_leaves = max_leaves or int(sizes.max())
    d, d_off = _torch(flat), _torch(off)
    roots = torch.full((n_trees, 4), SENTINEL, dtype=torch.int64, device=d.device)
    d_lv = torch.full((TS.levels_bound(flat.shape[0], n_trees, max_leaves, arity) + tail, 4), SENTINEL, dtype=torch.int64, device=d.device)
    ctx.merkle_forest_ragged_device(_tag(arity), d, d_off, n_trees, max_leaves, roots, d_lv, None, arity=arity)
    return d, d_off, roots, d_lv


def _update(ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots=None):
    """one update call -> (n_bad, n_hashed) as device tensors"""
    import torch
    k = len(tid)
    bad = torch.zeros(1, dtype=torch.int32, device=d.device)
    hashed = torch.zeros(1, dtype=torch.int64, device=d.device)
    ctx.merkle_forest_ragged_update_device(_tag(arity), d, d_off, n_trees, max_leaves, d_lv, _torch(np.asarray(tid, np.uint32)),
                                           _torch(np.asarray(lid, np.uint64)), _torch(new), k, d_roots=d_roots, d_n_bad=bad,
                                           d_n_hashed=hashed, arity=arity)
    return bad, hashed


def _distinct_pairs(sizes, rng, k, trees=None):
    """k distinct (tree, leaf) pairs of the trees `trees` (default: all), in random order"""
    trees = np.arange(len(sizes)) if trees is None else np.asarray(trees)
    tid = np.repeat(trees, np.asarray(sizes)[trees])
    lid = np.concatenate([np.arange(sizes[t]) for t in trees])
    pick = rng.choice(tid.size, size=min(k, tid.size), replace=False)
    return tid[pick], lid[pick]


def _check_against_fresh_build(ctx, oracle_mod, arity, flat, off, tid, lid, new, d, d_lv, d_roots, max_leaves=None):
    """after an update of the valid (tid, lid) with `new`: leaves, the whole d_levels (sentinel tail included) and the roots of the
    touched trees equal a fresh build of the modified leaves; every root equals the oracle's; untouched roots keep the sentinel"""
    import torch
    sizes = np.diff(off.astype(np.int64))
    want = flat.copy()
    want[off[tid].astype(np.int64) + np.asarray(lid, np.int64)] = new
    assert np.array_equal(_np(d), want)
    bound = TS.levels_bound(flat.shape[0], len(sizes), max_leaves or int(sizes.max()), arity)
    _, _, f_roots, f_lv = _forest(ctx, arity, want, off, max_leaves, tail=d_lv.shape[0] - bound)
    torch.cuda.synchronize()
    assert torch.equal(d_lv, f_lv)
    touched = np.zeros(len(sizes), bool)
    touched[np.asarray(tid)] = True
    got, fresh = _np(d_roots), _np(f_roots)
    assert np.array_equal(got[touched], fresh[touched])
    assert (got[~touched] == np.uint64(SENTINEL & (2 ** 64 - 1))).all()
    tree = _tree(oracle_mod, arity)
    for t in range(len(sizes)):
        if sizes[t] > 0:
            assert np.array_equal(fresh[t], tree(_tag(arity), want[int(off[t]):int(off[t + 1])])[0]), t
    return want, fresh


class Old:
    """a forest built on the device with its tree-major levels"""

    def __init__(self, ctx, arity, flat, off, max_leaves):
        import torch
        self.arity, self.flat, self.off, self.max_leaves, self.n_trees = arity, flat, np.asarray(off, np.uint64), max_leaves, len(off) - 1
        self.d, self.d_off = _torch(flat), _torch(self.off)
        self.roots = torch.full((self.n_trees, 4), SENTINEL, dtype=torch.int64, device=self.d.device)
        self.d_lv = torch.full((TS.levels_bound(flat.shape[0], self.n_trees, max_leaves, arity) + 3, 4), SENTINEL, dtype=torch.int64, device=self.d.device)
        ctx.merkle_forest_ragged_device(_tag(arity), self.d, self.d_off, self.n_trees, max_leaves, self.roots, self.d_lv, None, arity=arity)


def _outputs(arity, total, n_trees_new, max_new, tail=7):
    """sentinel-filled output buffers with `tail` scalars past what the call may use -> (leaves, offsets, levels, roots)"""
    import torch
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int64, device="cuda:0")  # noqa: E731
    return full(total + tail, 4), full(n_trees_new + 1 + tail), full(TS.levels_bound(total, n_trees_new, max_new, arity) + tail, 4), full(n_trees_new + tail, 4)


def _append(ctx, old, d_add, d_aoff, n_trees_new, max_new, out, bad=None, hashed=None):
    ctx.merkle_forest_ragged_append_device(_tag(old.arity), old.d, old.d_off, old.n_trees, old.max_leaves, old.d_lv, d_add, d_aoff, n_trees_new, max_new,
                                           out[0], out[1][:n_trees_new + 1], out[2], out[3][:n_trees_new], bad, hashed, arity=old.arity)


def _fresh(ctx, arity, M, old_flat, add, n_trees_new, max_new, like):
    """the reference: the model's new forest (leaves padded with the sentinel to the capacity of `like`), built afresh into
    sentinel-filled buffers of the same sizes -> (leaves, offsets, levels, roots)"""
    import torch
    leaves, offsets, levels, roots = (torch.full_like(t, SENTINEL) for t in like)
    want = model_leaves(M, old_flat, add)
    leaves[:want.shape[0]] = _torch(want)
    offsets[:n_trees_new + 1] = _torch(M["offsets_new"].astype(np.uint64))
    ctx.merkle_forest_ragged_device(_tag(arity), leaves, offsets[:n_trees_new + 1], n_trees_new, max_new, roots[:n_trees_new], levels, None, arity=arity)
    return leaves, offsets, levels, roots


class Grown(Old):
    """the outputs of an append, as the forest the next call reads"""

    def __init__(self, arity, out, n_trees, max_leaves):
        self.arity, self.n_trees, self.max_leaves = arity, n_trees, max_leaves
        self.d, self.d_off, self.d_lv, self.roots = out[0], out[1][:n_trees + 1], out[2], out[3][:n_trees]


def _single_extract(ctx, arity, n, d, d_lv, pos, cap=None, pad=0):
    """one extraction -> (leaves_out (k + pad, 4) numpy, the whole proof buffer (bound + pad, 4) numpy, proof_len, n_bad); the call
    sees the first k rows / the first `cap` (default: bound) rows only, the rest holds the sentinel"""
    import torch
    k = len(pos)
    bound = ctx.merkle_multiproof_bound(n, k, arity)
    cap = bound if cap is None else cap
    out = torch.full((k + pad, 4), SENTINEL, dtype=torch.int64, device=d.device)
    proof = torch.full((bound + pad, 4), SENTINEL, dtype=torch.int64, device=d.device)
    plen = torch.full((1,), -1, dtype=torch.int64, device=d.device)
    bad = torch.zeros(1, dtype=torch.int32, device=d.device)
    ctx.merkle_multiproof_device(d, n, d_lv if n > 1 else None, _torch(np.asarray(pos, np.uint32)), k, out[:k], proof[:cap] if cap else None,
                                 plen, d_n_bad=bad, arity=arity)
    ctx.sync()
    return _np(out), _np(proof), int(plen), int(bad)


def _single_verify(ctx, arity, n, pos, leaves, proof, proof_len, root):
    """one verification of numpy inputs -> (ok, root_out numpy or None when untouched, n_hashed, n_bad)"""
    import torch
    dev = "cuda:0"
    ok = torch.full((1,), 7, dtype=torch.uint8, device=dev)
    root_out = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
    hashed = torch.full((1,), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    d_proof = _torch(np.ascontiguousarray(proof, dtype=np.uint64)) if len(proof) else None
    ctx.merkle_multiproof_verify_device(_tag(arity), n, _torch(np.asarray(pos, np.uint32)), _torch(np.ascontiguousarray(leaves, dtype=np.uint64)),
                                        len(pos), d_proof, proof_len, _torch(np.ascontiguousarray(root, dtype=np.uint64)), ok,
                                        d_root_out=root_out, d_n_hashed=hashed, d_n_bad=bad, arity=arity)
    ctx.sync()
    r = _np(root_out)
    return int(ok), (None if (r == np.uint64(SENTINEL & (2 ** 64 - 1))).all() else r), int(hashed), int(bad)


def _median_ms(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _v2_rate(ctx, reps=7):
    """sum of depths / time of path_ragged on a mixed forest (2,000 trees log-uniform in [1, 4^6], 2^19 openings, the tree drawn
    uniformly), in levels per second"""
    import torch
    rng = np.random.default_rng(2)
    top = 4 ** 6
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), 2000))).astype(np.int64).clip(1, top)
    off = TS.offsets(sizes)
    d = torch.randint(0, 1 << 60, (int(off[-1]), 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(off)
    roots, d_lv = _build(ctx, 4, d, d_off, len(sizes), top)
    k = 1 << 19
    tid = rng.integers(0, len(sizes), k)
    lid = (rng.random(k) * sizes[tid]).astype(np.int64)
    o = _open(ctx, 4, d, d_off, len(sizes), top, d_lv, tid, lid)
    torch.cuda.synchronize()
    assert torch.equal(o["back"], roots[_torch(tid.astype(np.int64))])
    run = lambda: ctx.merkle_path_ragged_device(_tag(4), o["leaves"], o["sib"], o["pos"], o["dep"], o["D"], o["back"], k)  # noqa: E731
    run()
    ms = _median_ms(run, reps)
    levels = int(o["dep"].to(torch.int64).sum())
    return {"ms": ms, "levels_per_s": levels / ms * 1e3}
