#!/usr/bin/env python3
"""A forest of Merkle trees of different sizes in one call (p252_merkle{4,2}_forest_ragged_device) against the calls it replaces.

  python bench_tools/forest_ragged_bench.py [--reps 20] [--w2-trees 20000] [--per-tree 1000]

W1, equal sizes: 4,096 x 4^6 leaves (arity 4) and 4,096 x 2^12 leaves (arity 2), the ragged call against
p252_merkle{4,2}_forest_device, alternated in one process (median of --reps each); roots compared byte for byte.
W2, mixed sizes: --w2-trees seeded trees with leaf counts log-uniform in [1, 4^7]: one ragged call (median of --reps), useful
perm/s = sum of levels_len(n_t) / time, against one p252_merkle4_tree_device call per tree on the first --per-tree trees
(a SUBSET, reported per tree); the subset's roots compared byte for byte.  The shader clock is sampled around the run
(p252_clock_probe_device).  Prints one line per workload and a JSON summary last."""
import argparse
import ctypes
import json

import numpy as np

import _common as C
from testsupport import treeshape as TS


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--w1-trees", type=int, default=4096)
    ap.add_argument("--w2-trees", type=int, default=20000)
    ap.add_argument("--per-tree", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import _lib, levels_len
    from poseidon252_amd import merkle as M
    from poseidon252_amd.hash import _stream
    ctx = P.Context(0)
    L = _lib.lib()
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx)}

    # ---- W1: equal sizes ----
    for arity, per in ((4, 4 ** 6), (2, 2 ** 12)):
        tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        n_trees = a.w1_trees
        d = torch.randint(0, 1 << 60, (n_trees * per, 4), dtype=torch.int64, device=dev)
        d_off = torch.from_numpy(TS.offsets([per] * n_trees).view(np.int64)).to(dev)
        ra = torch.empty((n_trees, 4), dtype=torch.int64, device=dev)
        rb = torch.empty_like(ra)
        forest = lambda: ctx.merkle4_forest_device(tag, d, n_trees, per, ra, arity=arity)  # noqa: E731
        ragged = lambda: ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, per, rb, arity=arity)  # noqa: E731
        forest(), ragged()
        tf, tr = [], []
        for _ in range(a.reps):  # alternated
            tf.append(C.median_ms(forest, 1))
            tr.append(C.median_ms(ragged, 1))
        same = bool(torch.equal(ra, rb))
        perms = n_trees * levels_len(per, arity)
        mf, mr = float(np.median(tf)), float(np.median(tr))
        w = {"trees": n_trees, "leaves_per_tree": per, "perms": perms, "forest_ms": mf, "ragged_ms": mr,
             "forest_perm_s": perms / mf * 1e3, "ragged_perm_s": perms / mr * 1e3, "ragged_over_forest": mf / mr, "identical": same}
        res["w1_arity%d" % arity] = w
        print("W1 arity %d: %d x %d leaves  forest %.3f ms (%.3e perm/s)  ragged %.3f ms (%.3e perm/s)  ratio %.3f  identical %s"
              % (arity, n_trees, per, mf, w["forest_perm_s"], mr, w["ragged_perm_s"], mf / mr, same), flush=True)
        del d, d_off, ra, rb
        torch.cuda.empty_cache()

    # ---- W2: mixed sizes ----
    rng = np.random.default_rng(a.seed)
    top = 4 ** 7
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), a.w2_trees))).astype(np.int64).clip(1, top)
    off = TS.offsets(sizes)
    tag = M.merkle4_tag()
    d = torch.randint(0, 1 << 60, (int(off[-1]), 4), dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    roots = torch.empty((len(sizes), 4), dtype=torch.int64, device=dev)
    one = lambda: ctx.merkle_forest_ragged_device(tag, d, d_off, len(sizes), top, roots)  # noqa: E731
    one()
    t_one = C.median_ms(one, a.reps)
    perms = int(sum(levels_len(int(n), 4) for n in sizes))
    sub = min(a.per_tree, len(sizes))
    sub_roots = torch.empty((sub, 4), dtype=torch.int64, device=dev)
    tag_np = np.ascontiguousarray(tag, dtype=np.uint64)
    tp = tag_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    st = _stream(ctx)
    base = d.data_ptr()

    def each():
        for t in range(sub):
            rc = L.p252_merkle4_tree_device(ctx._h, tp, base + int(off[t]) * 32, int(sizes[t]), sub_roots[t].data_ptr(), None, st)
            assert rc == 0
    each()
    t_each = C.median_ms(each, max(1, min(a.reps, 3)))
    same = bool(torch.equal(sub_roots, roots[:sub]))
    w1 = res["w1_arity4"]["forest_perm_s"]
    w = {"trees": len(sizes), "leaves": int(off[-1]), "useful_perms": perms, "ragged_ms": t_one, "ragged_perm_s": perms / t_one * 1e3,
         "of_w1_forest_rate": perms / t_one * 1e3 / w1, "per_tree_subset": sub, "per_tree_subset_ms": t_each,
         "ms_per_tree_ragged": t_one / len(sizes), "ms_per_tree_single_calls": t_each / sub,
         "per_tree_speedup": (t_each / sub) / (t_one / len(sizes)), "subset_identical": same}
    res["w2"] = w
    print("W2: %d trees (log-uniform 1..4^7, %d leaves)  ragged %.3f ms, %.3e useful perm/s (%.3f of W1's forest rate)  "
          "per-tree calls on the first %d (subset): %.3f ms = %.4f ms/tree vs %.5f ms/tree  speedup %.1fx  identical %s"
          % (len(sizes), int(off[-1]), t_one, w["ragged_perm_s"], w["of_w1_forest_rate"], sub, t_each, t_each / sub, t_one / len(sizes),
             w["per_tree_speedup"], same), flush=True)
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
