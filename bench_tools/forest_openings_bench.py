#!/usr/bin/env python3
"""Openings out of a forest of trees of different sizes in one call (p252_merkle{4,2}_forest_ragged_openings_device,
p252_merkle{4,2}_path_ragged_device, p252_merkle{4,2}_forest_ragged_verify_device) against the calls they replace.

  python bench_tools/forest_openings_bench.py [--reps 10] [--openings 1048576] [--v2-trees 20000] [--per-tree 1000]

Every shape is warmed up; times are medians of --reps host wall clocks around calls that end in a device synchronise; the two
sides of a ratio alternate in the one process; outputs are compared byte for byte; the shader clock is probed before and after.
V1, equal depths: 4,096 trees x 4^6 leaves (arity 2: x 2^12), --openings openings: path_ragged against
p252_merkle{4,2}_path_batch_device on the same openings (useful perm/s = openings x depth / time), and the extraction's
algorithmic TB/s (96 + 96 + 1 bytes per (opening, level), arity 2: 32 + 32 + 1; + 64 per opening).
V2, mixed depths: --v2-trees trees with leaf counts log-uniform in [1, 4^7] (the W2 of forest_ragged_bench.py), the tree drawn
uniformly and the leaf uniformly inside it: sum of depths / time of path_ragged, sorted (this process) and with
P252_RAGGED_SORT=0 (a child process: the switch is read once), beside the bound (mean over waves of the wave's deepest lane) /
(mean depth) of the unsorted order, which needs no GPU.
Per tree (a SUBSET: the first --per-tree trees of V2, one opening each): one p252_merkle4_openings_device + one
p252_merkle4_verify_batch_device call per tree against one forest openings + one forest verify call.
Prints one line per workload and a JSON summary last."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

import _common as C
from testsupport import treeshape as TS


class Forest:
    """a built forest (tree-major levels) and k openings of it in caller-owned tensors"""

    def __init__(self, ctx, arity, sizes, max_leaves, tid, lid):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.arity, self.n_trees, self.max_leaves, self.k = ctx, arity, len(sizes), max_leaves, len(tid)
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        off = TS.offsets(sizes)
        n_leaves = int(off[-1])
        dev = torch.device("cuda:0")
        self.d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device=dev)
        self.d_off = C.dev(off)
        self.D = D = TS.depth(max_leaves, arity)
        self.roots = torch.empty((self.n_trees, 4), dtype=torch.int64, device=dev)
        self.d_lv = torch.empty((TS.levels_bound(n_leaves, self.n_trees, max_leaves, arity) + 1, 4), dtype=torch.int64, device=dev)
        ctx.merkle_forest_ragged_device(self.tag, self.d, self.d_off, self.n_trees, max_leaves, self.roots, self.d_lv, arity=arity)
        k = self.k
        self.d_tid, self.d_lid = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(lid, np.uint64))
        self.out = (torch.empty((k, 4), dtype=torch.int64, device=dev), torch.empty((k, D, arity - 1, 4), dtype=torch.int64, device=dev),
                    torch.empty((k, D), dtype=torch.uint8, device=dev), torch.empty((k,), dtype=torch.uint8, device=dev))
        self.back = torch.empty((k, 4), dtype=torch.int64, device=dev)
        self.ok = torch.empty((k,), dtype=torch.uint8, device=dev)

    def extract(self, k=None):
        self.ctx.merkle_forest_ragged_openings_device(self.d, self.d_off, self.n_trees, self.max_leaves, self.d_lv, self.d_tid, self.d_lid,
                                                      self.k if k is None else k, out=self.out, arity=self.arity)

    def rehash(self):
        o = self.out
        self.ctx.merkle_path_ragged_device(self.tag, o[0], o[1], o[2], o[3], self.D, self.back, self.k, arity=self.arity)

    def verify(self, k=None):
        o = self.out
        self.ctx.merkle_forest_ragged_verify_device(self.tag, o[0], o[1], o[2], o[3], self.D, self.d_tid, self.roots, self.n_trees, self.ok,
                                                    self.k if k is None else k, arity=self.arity)


def _v2_draw(a):
    rng = np.random.default_rng(a.seed)
    top = 4 ** 7
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), a.v2_trees))).astype(np.int64).clip(1, top)
    tid = rng.integers(0, len(sizes), a.openings)
    tid[:min(a.per_tree, len(sizes), a.openings)] = np.arange(min(a.per_tree, len(sizes), a.openings))  # the per-tree subset comes first
    lid = (rng.random(a.openings) * sizes[tid]).astype(np.int64)
    return sizes, top, tid, lid


def _v2(ctx, a):
    import torch
    sizes, top, tid, lid = _v2_draw(a)
    f = Forest(ctx, 4, sizes, top, tid, lid)
    f.extract(), f.rehash(), f.verify()
    torch.cuda.synchronize()
    same = bool(torch.equal(f.back, f.roots[C.dev(tid.astype(np.int64))])) and int(f.ok.sum()) == f.k
    ms = C.median_ms(f.rehash, a.reps)
    depths = TS.depth(sizes, 4)[tid]
    waves = depths[:depths.size // 64 * 64].reshape(-1, 64)
    return f, {"trees": len(sizes), "openings": f.k, "levels": int(depths.sum()), "mean_depth": float(depths.mean()),
               "rehash_ms": ms, "levels_per_s": float(depths.sum()) / ms * 1e3, "roots_match_the_build": same,
               "unsorted_bound_wave_max_over_mean": float(waves.max(axis=1).mean() / depths.mean()),
               "depth_histogram": np.bincount(depths, minlength=8).tolist()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--openings", type=int, default=1 << 20)
    ap.add_argument("--v1-trees", type=int, default=4096)
    ap.add_argument("--v2-trees", type=int, default=20000)
    ap.add_argument("--per-tree", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--v2-only", action="store_true", help="(internal: the P252_RAGGED_SORT=0 child) V2's re-hash alone, JSON only")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import _lib
    from poseidon252_amd.hash import _stream
    ctx = P.Context(0)
    if a.v2_only:
        print(json.dumps(_v2(ctx, a)[1]))
        return
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx)}

    # ---- V1: equal depths ----
    for arity, per in ((4, 4 ** 6), (2, 2 ** 12)):
        rng = np.random.default_rng(a.seed + arity)
        k = a.openings
        f = Forest(ctx, arity, [per] * a.v1_trees, per, rng.integers(0, a.v1_trees, k), rng.integers(0, per, k))
        D = f.D
        exp = torch.empty_like(f.back)
        fixed_fn = ctx.merkle4_path_batch_device if arity == 4 else ctx.merkle2_path_batch_device
        fixed = lambda: fixed_fn(f.tag, f.out[0], f.out[1], f.out[2], D, exp, k)  # noqa: E731
        f.extract(), f.rehash(), fixed(), f.verify()
        tf, tr = [], []
        for _ in range(a.reps):  # alternated
            tf.append(C.median_ms(fixed, 1))
            tr.append(C.median_ms(f.rehash, 1))
        same = bool(torch.equal(exp, f.back)) and int(f.ok.sum()) == k
        t_ext, t_ver = C.median_ms(f.extract, a.reps), C.median_ms(f.verify, a.reps)
        small = min(1000, k)
        t_ext_small = C.median_ms(lambda: f.extract(small), a.reps)
        mf, mr = float(np.median(tf)), float(np.median(tr))
        per_level = (96 + 96 + 1) if arity == 4 else (32 + 32 + 1)
        ext_bytes = k * (D * per_level + 64)
        w = {"trees": a.v1_trees, "leaves_per_tree": per, "openings": k, "depth": D, "perms": k * D, "fixed_ms": mf, "ragged_ms": mr,
             "fixed_perm_s": k * D / mf * 1e3, "ragged_perm_s": k * D / mr * 1e3, "ragged_over_fixed": mf / mr, "identical": same,
             "extract_ms": t_ext, "extract_algorithmic_tb_s": ext_bytes / t_ext * 1e3 / 1e12, "extract_%d_openings_ms" % small: t_ext_small,
             "verify_ms": t_ver}
        res["v1_arity%d" % arity] = w
        print("V1 arity %d: %d openings of depth %d  fixed %.3f ms (%.3e perm/s)  ragged %.3f ms (%.3e perm/s)  ratio %.3f  identical %s  "
              "extract %.3f ms (%.2f TB/s algorithmic; %d openings: %.3f ms)  verify %.3f ms"
              % (arity, k, D, mf, w["fixed_perm_s"], mr, w["ragged_perm_s"], mf / mr, same, t_ext, w["extract_algorithmic_tb_s"], small,
                 t_ext_small, t_ver), flush=True)
        del f, exp
        torch.cuda.empty_cache()

    # ---- V2: mixed depths, sorted here and unsorted in a child process ----
    f, w = _v2(ctx, a)
    w["of_v1_fixed_rate"] = w["levels_per_s"] / res["v1_arity4"]["fixed_perm_s"]
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--v2-only", "--reps", str(a.reps), "--openings", str(a.openings),
                            "--v2-trees", str(a.v2_trees), "--per-tree", str(a.per_tree), "--seed", str(a.seed)],
                           env=dict(os.environ, P252_RAGGED_SORT="0"), capture_output=True, text=True, timeout=1200)
    if child.returncode == 0:
        u = json.loads(child.stdout.strip().splitlines()[-1])
        w["unsorted_rehash_ms"], w["unsorted_levels_per_s"] = u["rehash_ms"], u["levels_per_s"]
        w["sorted_over_unsorted"] = w["levels_per_s"] / u["levels_per_s"]
    else:
        w["unsorted_error"] = child.stderr[-500:]
    res["v2"] = w
    print("V2: %d trees, %d openings, mean depth %.2f  sorted %.3f ms = %.3e levels/s (%.3f of V1's fixed-depth rate)  unsorted %s ms  "
          "sorted/unsorted %s (bound of the generated depths %.3f)"
          % (w["trees"], w["openings"], w["mean_depth"], w["rehash_ms"], w["levels_per_s"], w["of_v1_fixed_rate"],
             w.get("unsorted_rehash_ms"), w.get("sorted_over_unsorted"), w["unsorted_bound_wave_max_over_mean"]), flush=True)

    # ---- per tree: the first --per-tree trees of V2, one opening each (a SUBSET) ----
    sizes, top, tid, lid = _v2_draw(a)
    sub = min(a.per_tree, len(sizes), a.openings)
    L = _lib.lib()
    from poseidon252_amd import levels_len
    lo = np.zeros(sub + 1, dtype=np.int64)
    np.cumsum([levels_len(int(n), 4) for n in sizes[:sub]], out=lo[1:])
    off = TS.offsets(sizes)
    import ctypes
    tp = np.ascontiguousarray(f.tag, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    st = _stream(ctx)
    idx32 = C.dev(lid[:sub].astype(np.uint32))
    one_out = torch.zeros((sub, 4), dtype=torch.int64, device="cuda:0")
    one_sib = torch.zeros((sub, f.D, 3, 4), dtype=torch.int64, device="cuda:0")
    one_pos = torch.zeros((sub, f.D), dtype=torch.uint8, device="cuda:0")
    one_ok = torch.zeros(sub, dtype=torch.uint8, device="cuda:0")
    deps = [TS.depth(int(n), 4) for n in sizes[:sub]]

    def each():
        for t in range(sub):
            n, dp = int(sizes[t]), deps[t]
            rc = L.p252_merkle4_openings_device(ctx._h, f.d.data_ptr() + int(off[t]) * 32, n, f.d_lv.data_ptr() + int(lo[t]) * 32 if dp else None,
                                                idx32.data_ptr() + 4 * t, 1, one_out.data_ptr() + 32 * t,
                                                one_sib.data_ptr() + 96 * f.D * t if dp else None, one_pos.data_ptr() + f.D * t if dp else None,
                                                None, st)
            assert rc == 0
            rc = L.p252_merkle4_verify_batch_device(ctx._h, tp, one_out.data_ptr() + 32 * t, one_sib.data_ptr() + 96 * f.D * t if dp else None,
                                                    one_pos.data_ptr() + f.D * t if dp else None, dp, f.roots.data_ptr() + 32 * t,
                                                    one_ok.data_ptr() + t, 1, st)
            assert rc == 0

    def one():
        f.extract(sub)
        f.verify(sub)
    each(), one()
    t_each, t_one = C.median_ms(each, max(1, min(a.reps, 3))), C.median_ms(one, a.reps)
    same = int(one_ok.sum()) == sub and int(f.ok[:sub].sum()) == sub and bool(torch.equal(one_out, f.out[0][:sub]))
    res["per_tree"] = {"subset": sub, "single_calls_ms": t_each, "forest_calls_ms": t_one, "ms_per_tree_single_calls": t_each / sub,
                       "ms_per_tree_forest_calls": t_one / sub, "speedup": t_each / t_one, "identical": same}
    print("per tree (first %d trees of V2, a subset, one opening each): %.3f ms in %d + %d single-tree calls, %.3f ms in one openings + one "
          "verify call: %.1fx  identical %s" % (sub, t_each, sub, sub, t_one, t_each / t_one, same), flush=True)
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
