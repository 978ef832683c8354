#!/usr/bin/env python3
"""Leaves appended to the trees of a built forest (p252_merkle{4,2}_forest_ragged_append_device_into: clean nodes moved, dirty ones
hashed once) against a fresh p252_merkle{4,2}_forest_ragged_device build of the same new forest, timed in the same run.

  python bench_tools/forest_append_bench.py [--reps 9] [--out profiles/forest_append.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock
inside the bracket); the two sides of a ratio alternate in the one process; the results are compared byte for byte; the shader
clock is probed before and after.
A, one tree: 4^12 leaves (arity 4) and 2^24 leaves (arity 2) plus 2^0, 2^10, 2^16, 2^20 appended leaves.
B, many trees: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7) with 1 to 16
leaves appended to EVERY tree.  C: the same with leaves appended to 1 % of the trees.
R, the relocation alone: a compaction copy (nothing appended: the two relocation kernels and the bookkeeping, no digest) of A's
trees; bytes read plus written per second, beside the rate of a device-to-device copy of the same bytes in the same run
(bench_tools/copy_rate.hip measures the plain-copy rate of the box on its own).
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Case
# (the numpy model of the call lived in this module once: its names stay importable from here)
from testsupport.forestappend import forest_append_model, good_leaf_counts, model_leaves  # noqa: F401
from testsupport.treeshape import level_widths  # noqa: F401


def _measure(case, reps):
    import torch
    case.append(count=True)
    case.rebuild()
    same = case.identical()
    hashed = int(case.hashed)
    t_app, t_build = C.alternate([case.append, case.rebuild], reps, C.event_ms)
    torch.cuda.synchronize()
    return {"append_ms": t_app, "rebuild_ms": t_build, "ratio": t_build / t_app, "digests": hashed, "identical": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_append.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "a": [], "r": []}
    say("python bench_tools/forest_append_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))

    # ---- A: one tree; R: its compaction copy ----
    for arity, n in ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24)):
        for m in ([1, 1 << 6, 1 << 10] if a.quick else [1, 1 << 10, 1 << 16, 1 << 20]):
            c = Case(ctx, arity, [n], [m])
            r = dict(_measure(c, a.reps), arity=arity, leaves=n, appended=m)
            res["a"].append(r)
            say("A arity %d, %d leaves + %d: append %.3f ms (%d digests)  fresh build %.3f ms  build/append %.2f  identical %s"
                % (arity, n, m, r["append_ms"], r["digests"], r["rebuild_ms"], r["ratio"], r["identical"]))
            del c
            torch.cuda.empty_cache()
        c = Case(ctx, arity, [n], [0])
        moved = 2 * 32 * (n + int(c.lv.shape[0]))  # every leaf and every node of the tree, read and written
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        c.append(), dst.copy_(src)
        t_move, t_copy = C.alternate([c.append, lambda: dst.copy_(src)], a.reps, C.event_ms)
        r = {"arity": arity, "leaves": n, "bytes": moved, "compaction_ms": t_move, "copy_ms": t_copy, "compaction_gbs": moved / t_move / 1e6,
             "copy_gbs": moved / t_copy / 1e6}
        res["r"].append(r)
        say("R arity %d, %d leaves, nothing appended: %.3f ms for %d bytes read + written = %.0f GB/s (bookkeeping launches included)  "
            "device-to-device copy of the same bytes %.3f ms = %.0f GB/s  copy/compaction %.2f"
            % (arity, n, t_move, moved, r["compaction_gbs"], t_copy, r["copy_gbs"], t_copy / t_move))
        del c, src, dst
        torch.cuda.empty_cache()

    # ---- B, C: the mixed forest ----
    rng = np.random.default_rng(a.seed)
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    every = rng.integers(1, 17, n_trees)
    few = np.where(rng.random(n_trees) < 0.01, every, 0)
    for name, adds in (("b", every), ("c", few)):
        c = Case(ctx, 4, sizes, adds)
        r = dict(_measure(c, a.reps), trees=n_trees, leaves=int(sizes.sum()), appended=int(adds.sum()), trees_appended_to=int((adds > 0).sum()))
        res[name] = r
        say("%s: %d trees (log-uniform 1..4^7, %d leaves), %d leaves appended to %d trees: append %.3f ms (%d digests)  fresh build %.3f ms  "
            "build/append %.2f  identical %s" % (name.upper(), n_trees, r["leaves"], r["appended"], r["trees_appended_to"], r["append_ms"], r["digests"],
                                                 r["rebuild_ms"], r["ratio"], r["identical"]))
        del c
        torch.cuda.empty_cache()
    for arity in (4, 2):
        rows = [r for r in res["a"] if r["arity"] == arity]
        lose = [r for r in rows if r["ratio"] < 1.0]
        say("arity %d: a fresh build is as quick from %s appended leaves of %d" % (arity, ("%d (1/%d of the tree)" % (lose[0]["appended"], rows[0]["leaves"] // lose[0]["appended"])) if lose else "none of the sweep", rows[0]["leaves"]))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
