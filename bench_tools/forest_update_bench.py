#!/usr/bin/env python3
"""Leaf updates anywhere in a forest of trees of different sizes in one call (p252_merkle{4,2}_forest_ragged_update_device, every
dirty node hashed once) against the calls it replaces.

  python bench_tools/forest_update_bench.py [--reps 9] [--out profiles/forest_update.txt] [--quick]

Every shape is warmed up; times are medians of --reps host wall clocks around calls that end in a device synchronise; the two
sides of a ratio alternate in the one process; the update list is re-applied each repetition (re-writing the same values does
the same work); results are compared byte for byte; the shader clock is probed before and after.
U1, de-duplication: ONE arity-4 tree of 4^12 leaves, k = 2^10, 2^16, 2^20 distinct random leaves (seed 1), and the GPU test's
size (4^11 leaves, k = 2^18): the forest call (a forest of one tree) against p252_merkle4_update_device on the same updates.
Digest counts of both from numpy.
U2, one call against per-tree calls: the W2 forest of forest_ragged_bench.py (--u2-trees trees, leaf counts log-uniform in
[1, 4^7], seed 7), one update per tree at a random leaf: the forest call, a loop of p252_merkle4_update_device over the blocks
(timed on the first --per-tree trees, a SUBSET, and reported per tree), and a full merkle_forest_ragged_device rebuild.
U3, crossover: on U1's tree, k swept in powers of 4 up to N: the forest call against a full rebuild.
Arity 2: one tree of 2^24 leaves, k = 2^10, 2^16, 2^20, against the rebuild (there is no older arity-2 update).
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT
from testsupport import treeshape as TS
from testsupport.forestupdate import dirty_nodes


class Forest(C.Forest):
    def updater(self, tid, lid, seed=3):
        """the forest call on (tid, lid) with random new leaves -> (callable, the new leaves, d_n_hashed)"""
        import torch
        k = len(tid)
        d_tid, d_lid = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(lid, np.uint64))
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        d_new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device="cuda:0", generator=g)
        hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")

        def call(count=False):
            self.ctx.merkle_forest_ragged_update_device(self.tag, self.d, self.d_off, self.n_trees, self.max_leaves, self.d_lv, d_tid, d_lid,
                                                        d_new, k, d_roots=self.roots, d_n_hashed=hashed if count else None, arity=self.arity)
        return call, d_new, hashed


def _u1(ctx, n, ks, reps, say):
    """one arity-4 tree of n leaves: the forest call against p252_merkle4_update_device for each k"""
    import torch
    f = Forest(ctx, 4, [n], n)
    d_b, lv_b, root_b = f.d.clone(), f.d_lv.clone(), torch.zeros((1, 4), dtype=torch.int64, device="cuda:0")
    rows = []
    for k in ks:
        lid = np.random.default_rng(1).choice(n, k, replace=False)
        new, d_new, hashed = f.updater(np.zeros(k, np.int64), lid)
        d_idx = C.dev(lid.astype(np.uint32))
        old = lambda: ctx.merkle4_update_device(f.tag, d_b, n, lv_b, d_idx, d_new, k, d_root=root_b)  # noqa: E731
        new(count=True), old()
        torch.cuda.synchronize()
        same = bool(torch.equal(f.d, d_b)) and bool(torch.equal(f.d_lv[:lv_b.shape[0]], lv_b)) and bool(torch.equal(f.roots, root_b))
        t_old, t_new = C.alternate([old, new], reps, C.once_ms)
        dirty, per_level = dirty_nodes([n], np.zeros(k, np.int64), lid, 4), k * TS.depth(n, 4)
        rows.append({"leaves": n, "k": k, "per_level_ms": t_old, "once_ms": t_new, "ratio": t_old / t_new, "digests_per_level_call": per_level,
                     "digests_once": dirty, "digests_counted_on_device": int(hashed), "count_ratio": per_level / dirty, "identical": same})
        say("U1 4^%d leaves, k = 2^%d: p252_merkle4_update_device %.3f ms (%d digests)  forest update %.3f ms (%d digests, %d counted on the "
            "device)  ratio %.3f (digest counts %.2f)  identical %s"
            % (TS.depth(n, 4), int(np.log2(k)), t_old, per_level, t_new, dirty, int(hashed), t_old / t_new, per_level / dirty, same))
    return f, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--u2-trees", type=int, default=20000)
    ap.add_argument("--per-tree", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_update.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^9-leaf tree, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import ctypes
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import _lib, levels_len
    from poseidon252_amd.hash import _stream
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx)}
    say("python bench_tools/forest_update_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))

    # ---- U1: de-duplication ----
    n1 = 4 ** 9 if a.quick else 4 ** 12
    ks = [1 << 6, 1 << 10, 1 << 14] if a.quick else [1 << 10, 1 << 16, 1 << 20]
    f, res["u1"] = _u1(ctx, n1, ks, a.reps, say)

    # ---- U3: crossover against a full rebuild, on U1's tree ----
    res["u3"] = []
    k = 1
    while k <= n1:
        lid = np.random.default_rng(1).choice(n1, k, replace=False)
        new, _, _ = f.updater(np.zeros(k, np.int64), lid)
        new(), f.build()
        t_new, t_build = C.alternate([new, f.build], a.reps, C.once_ms)
        res["u3"].append({"k": k, "update_ms": t_new, "rebuild_ms": t_build, "ratio": t_build / t_new})
        say("U3 4^%d leaves, k = 4^%d (N/%d): forest update %.3f ms  full rebuild %.3f ms  rebuild/update %.3f"
            % (TS.depth(n1, 4), TS.depth(k, 4), n1 // k, t_new, t_build, t_build / t_new))
        k *= 4
    wins = [r["k"] for r in res["u3"] if r["ratio"] < 1.0]
    res["u3_rebuild_wins_from_k"] = wins[0] if wins else None
    say("U3: rebuilding wins from k = %s of N = %d" % (wins[0] if wins else "none of the sweep", n1))
    del f
    torch.cuda.empty_cache()
    if not a.quick:  # the GPU test's size
        f, rows = _u1(ctx, 4 ** 11, [1 << 18], a.reps, say)
        res["u1"] += rows
        del f
        torch.cuda.empty_cache()

    # ---- U2: one call against per-tree calls and against a rebuild ----
    rng = np.random.default_rng(a.seed)
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.u2_trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    f = Forest(ctx, 4, sizes, top)
    tid = np.arange(n_trees)
    lid = (rng.random(n_trees) * sizes).astype(np.int64)
    new, d_new, hashed = f.updater(tid, lid)
    sub = min(a.per_tree, n_trees)
    lo = np.zeros(n_trees + 1, dtype=np.int64)
    np.cumsum([levels_len(int(n), 4) for n in sizes], out=lo[1:])
    L = _lib.lib()
    tp = np.ascontiguousarray(f.tag, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    st = _stream(ctx)
    d_b, lv_b, roots_b = f.d.clone(), f.d_lv.clone(), f.roots.clone()
    idx32 = C.dev(lid.astype(np.uint32))

    def each():
        for t in range(sub):
            n = int(sizes[t])
            rc = L.p252_merkle4_update_device(ctx._h, tp, d_b.data_ptr() + int(f.off[t]) * 32, n, lv_b.data_ptr() + int(lo[t]) * 32 if n > 1 else None,
                                              idx32.data_ptr() + 4 * t, d_new.data_ptr() + 32 * t, 1, roots_b.data_ptr() + 32 * t, st)
            assert rc == 0
    new(count=True), each()
    torch.cuda.synchronize()
    same = (bool(torch.equal(f.roots[:sub], roots_b[:sub])) and bool(torch.equal(f.d_lv[:int(lo[sub])], lv_b[:int(lo[sub])]))
            and bool(torch.equal(f.d[:int(f.off[sub])], d_b[:int(f.off[sub])])))
    t_new, t_build = C.alternate([new, f.build], a.reps, C.once_ms)
    t_each = float(np.median([C.once_ms(each) for _ in range(max(1, min(a.reps, 3)))]))
    dirty, all_nodes = dirty_nodes(sizes, tid, lid, 4), int(sum(levels_len(int(n), 4) for n in sizes))
    res["u2"] = {"trees": n_trees, "leaves": int(sizes.sum()), "updates": n_trees, "update_ms": t_new, "rebuild_ms": t_build,
                 "per_tree_subset": sub, "per_tree_subset_ms": t_each, "ms_per_tree_single_calls": t_each / sub, "ms_per_tree_forest_call": t_new / n_trees,
                 "per_tree_speedup": (t_each / sub) / (t_new / n_trees), "rebuild_over_update": t_build / t_new, "digests_update": dirty,
                 "digests_counted_on_device": int(hashed), "digests_rebuild": all_nodes, "subset_identical": same}
    say("U2: %d trees (log-uniform 1..4^7, %d leaves), one update per tree: forest update %.3f ms (%d digests, %d counted on the device)  "
        "per-tree p252_merkle4_update_device calls on the first %d (subset): %.3f ms = %.4f ms/tree vs %.5f ms/tree: %.1fx  "
        "full rebuild %.3f ms (%d digests): %.1fx  identical %s"
        % (n_trees, int(sizes.sum()), t_new, dirty, int(hashed), sub, t_each, t_each / sub, t_new / n_trees, res["u2"]["per_tree_speedup"],
           t_build, all_nodes, t_build / t_new, same))
    del f, d_b, lv_b
    torch.cuda.empty_cache()

    # ---- arity 2 ----
    n2 = 2 ** 16 if a.quick else 2 ** 24
    f = Forest(ctx, 2, [n2], n2)
    res["arity2"] = []
    for k in ([1 << 6, 1 << 12] if a.quick else [1 << 10, 1 << 16, 1 << 20]):
        lid = np.random.default_rng(1).choice(n2, k, replace=False)
        new, _, hashed = f.updater(np.zeros(k, np.int64), lid)
        new(count=True)
        fresh_roots, fresh_lv = f.roots.clone(), f.d_lv.clone()
        f.build()
        torch.cuda.synchronize()
        same = bool(torch.equal(f.roots, fresh_roots)) and bool(torch.equal(f.d_lv[:n2 - 1], fresh_lv[:n2 - 1]))
        t_new, t_build = C.alternate([new, f.build], a.reps, C.once_ms)
        dirty = dirty_nodes([n2], np.zeros(k, np.int64), lid, 2)
        res["arity2"].append({"leaves": n2, "k": k, "update_ms": t_new, "rebuild_ms": t_build, "ratio": t_build / t_new, "digests_once": dirty,
                              "digests_counted_on_device": int(hashed), "digests_rebuild": n2 - 1, "identical": same})
        say("arity 2, 2^%d leaves, k = 2^%d: forest update %.3f ms (%d digests, %d counted on the device; k per level would be %d)  "
            "full rebuild %.3f ms (%d digests)  rebuild/update %.3f  identical %s"
            % (TS.depth(n2, 2), int(np.log2(k)), t_new, dirty, int(hashed), k * TS.depth(n2, 2), t_build, n2 - 1, t_build / t_new, same))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
