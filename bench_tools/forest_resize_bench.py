#!/usr/bin/env python3
"""A built forest rolled back, and forward again, in one call (p252_merkle{4,2}_forest_ragged_resize_device_into: every tree cut to
its first k_t leaves, then appended to; clean nodes moved, dirty ones hashed once) against a fresh
p252_merkle{4,2}_forest_ragged_device build of the same new forest, timed in the same run.

  python bench_tools/forest_resize_bench.py [--reps 9] [--out profiles/forest_resize.txt] [--quick]

The method is forest_append_bench.py's: every shape is warmed up; a time is the median of --reps launches, each between two device
events on the stream; the two sides of a ratio alternate in the one process; the results are compared byte for byte; the shader
clock is probed before and after.
A, one tree: 4^12 leaves (arity 4) and 2^24 leaves (arity 2) rolled back by 2^0, 2^8, 2^16, 2^20 leaves.
B, many trees: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7) with 1 to 16
leaves removed from EVERY tree (never more than the tree has).  C: the same with leaves removed from 1 % of the trees.
G, a reorg of B's forest: r_t leaves come off and r_t other leaves go on in one call, against the two-call sequence (a resize that
only cuts, then an append to its result).
R, the relocation alone: A's trees through the same call with every kept count at the tree's size (nothing is cut, so every leaf and
node moves and no digest finds work, but the whole launch sequence runs — the call cannot know that on the host); bytes read plus
written per second, beside a device-to-device copy of the same bytes in the same run.  The one-leaf rollback's time less this one's
is what its one-node digest launches, one per level, cost: the fixed cost of a rollback is the sum.
P, the append path with the library named by P252_LIB_PATH: forest_append_bench.py's two headline cases (one 4^12-leaf tree + 2^16
leaves; 20,000 mixed trees, leaves appended to every tree), append time only.  bench_tools/ab_variants.sh style: run this tool with
--append-only --label NAME once per library, alternating, and compare the medians with the spread one library shows against itself.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Case
from testsupport import treeshape as TS
# (the numpy model of the call lived in this module once: its names stay importable from here)
from testsupport.forestappend import KEEP_ALL, forest_resize_model  # noqa: F401


class ResizeCase(Case):
    """_common.Case with a kept count per tree: the resize, and the fresh build of its result"""

    def __init__(self, ctx, arity, sizes, cuts, adds):
        Case.__init__(self, ctx, arity, sizes, adds)
        sizes, cuts = np.asarray(sizes, dtype=np.int64), np.asarray(cuts, dtype=np.int64)
        self.d_keep = C.dev(sizes - cuts)
        self.resize_call = ctx.merkle4_forest_ragged_resize_device if arity == 4 else ctx.merkle2_forest_ragged_resize_device

    def append(self, count=False):  # (Case's name for the call under test: _measure and rebuild use it)
        self.resize_call(self.tag, self.d, self.d_off, self.T, self.max_old, self.lv, self.d_keep, self.d_add, self.d_aoff, self.T, self.max_new,
                         self.a_leaves, self.a_off, self.a_lv, self.a_roots, None, self.hashed if count else None)

    def identical(self):
        """roots, and the used part of the levels (the buffers are sized for the uncut forest)"""
        import torch
        torch.cuda.synchronize()
        used = int(TS.levels_len(np.diff(self.a_off.cpu().numpy()), self.arity).sum())
        return bool(torch.equal(self.a_roots, self.b_roots)) and bool(torch.equal(self.a_lv[:used], self.b_lv[:used]))


def _measure(case, reps):
    import torch
    case.hashed.zero_()
    case.append(count=True)
    case.rebuild()
    same = case.identical()
    hashed = int(case.hashed)
    t_call, t_build = C.alternate([case.append, case.rebuild], reps, C.event_ms)
    torch.cuda.synchronize()
    return {"resize_ms": t_call, "rebuild_ms": t_build, "ratio": t_build / t_call, "digests": hashed, "identical": same}


def _mixed(seed, n_trees):
    rng = np.random.default_rng(seed)
    top = 4 ** 7
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    every = rng.integers(1, 17, n_trees)
    few = np.where(rng.random(n_trees) < 0.01, every, 0)
    return sizes, every, few


def _append_only(ctx, a, say):
    """P: forest_append_bench.py's two headline cases, the append alone"""
    import torch
    out = {}
    sizes, every, _ = _mixed(a.seed, 2000 if a.quick else a.trees)
    for name, case in (("one_tree", lambda: Case(ctx, 4, [4 ** 8 if a.quick else 4 ** 12], [1 << 10 if a.quick else 1 << 16])),
                       ("mixed", lambda: Case(ctx, 4, sizes, every))):
        c = case()
        c.append()
        (t,) = C.alternate([c.append], a.reps, C.event_ms)
        out[name] = t
        del c
        torch.cuda.empty_cache()
    say("P append path, library %s: one tree + 2^16 leaves %.4f ms   mixed forest, every tree %.4f ms"
        % (a.label or os.environ.get("P252_LIB_PATH", "(the package's own)"), out["one_tree"], out["mixed"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_resize.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2,000 trees): a check of the tool, not a measurement")
    ap.add_argument("--append-only", action="store_true", help="only P, the append path of the library P252_LIB_PATH names; appends its line to --out")
    ap.add_argument("--label", default=None, help="with --append-only: the name of that library in the line (default: its path)")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if a.append_only:
        res = {"p": _append_only(ctx, a, say)}
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
        print(json.dumps(res))
        return
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "a": [], "r": []}
    say("python bench_tools/forest_resize_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))

    # ---- A: one tree rolled back; R: the relocation of its one-leaf rollback ----
    for arity, n in ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24)):
        for r in ([1, 1 << 4, 1 << 10] if a.quick else [1, 1 << 8, 1 << 16, 1 << 20]):
            c = ResizeCase(ctx, arity, [n], [r], [0])
            row = dict(_measure(c, a.reps), arity=arity, leaves=n, removed=r)
            res["a"].append(row)
            say("A arity %d, %d leaves - %d: resize %.3f ms (%d digests)  fresh build %.3f ms  build/resize %.2f  identical %s"
                % (arity, n, r, row["resize_ms"], row["digests"], row["rebuild_ms"], row["ratio"], row["identical"]))
            del c
            torch.cuda.empty_cache()
        c = ResizeCase(ctx, arity, [n], [0], [0])
        moved = 2 * 32 * (n + int(c.lv.shape[0]))  # every leaf and every node of the tree, read and written
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        c.append(count=True), dst.copy_(src)
        t_move, t_copy = C.alternate([c.append, lambda: dst.copy_(src)], a.reps, C.event_ms)
        one_leaf = [x for x in res["a"] if x["arity"] == arity and x["removed"] == 1][0]["resize_ms"]
        rr = {"arity": arity, "leaves": n, "bytes": moved, "relocation_ms": t_move, "copy_ms": t_copy, "relocation_tbs": moved / t_move / 1e9,
              "copy_tbs": moved / t_copy / 1e9, "digests": int(c.hashed), "one_leaf_rollback_ms": one_leaf, "one_leaf_digest_launches_ms": one_leaf - t_move}
        res["r"].append(rr)
        say("R arity %d, %d leaves, every kept count = the size: %.3f ms (%d digests) for %d bytes read + written = %.2f TB/s (every launch of the call "
            "included)  device-to-device copy of the same bytes %.3f ms = %.2f TB/s  copy/relocation %.2f  the one-leaf rollback above less this: "
            "%.3f ms in %d one-node digest launches" % (arity, n, t_move, rr["digests"], moved, rr["relocation_tbs"], t_copy, rr["copy_tbs"], t_copy / t_move,
                                                       rr["one_leaf_digest_launches_ms"], TS.depth(n - 1, arity)))
        del c, src, dst
        torch.cuda.empty_cache()

    # ---- B, C: the mixed forest; G: a reorg of it ----
    n_trees = 2000 if a.quick else a.trees
    sizes, every, few = _mixed(a.seed, n_trees)
    for name, cuts in (("b", np.minimum(every, sizes)), ("c", np.minimum(few, sizes))):
        c = ResizeCase(ctx, 4, sizes, cuts, np.zeros(n_trees, dtype=np.int64))
        row = dict(_measure(c, a.reps), trees=n_trees, leaves=int(sizes.sum()), removed=int(cuts.sum()), trees_cut=int((cuts > 0).sum()))
        res[name] = row
        say("%s: %d trees (log-uniform 1..4^7, %d leaves), %d leaves removed from %d trees: resize %.3f ms (%d digests)  fresh build %.3f ms  "
            "build/resize %.2f  identical %s" % (name.upper(), n_trees, row["leaves"], row["removed"], row["trees_cut"], row["resize_ms"], row["digests"],
                                                 row["rebuild_ms"], row["ratio"], row["identical"]))
        del c
        torch.cuda.empty_cache()
    cuts = np.minimum(every, sizes)
    one = ResizeCase(ctx, 4, sizes, cuts, cuts)        # r_t off, r_t on, one call
    cut = ResizeCase(ctx, 4, sizes, cuts, np.zeros(n_trees, dtype=np.int64))  # two calls: the cut ..
    cut.d.copy_(one.d)                                 # (a Case draws its own leaves: the two sides need the same old forest)
    cut.lv.copy_(one.lv)
    cut.append()
    app = ctx.merkle4_forest_ragged_append_device             # .. and an append to its result
    two_leaves, two_lv, two_roots = torch.zeros_like(one.a_leaves), torch.zeros_like(one.a_lv), torch.zeros_like(one.a_roots)
    two_off = torch.zeros_like(one.a_off)

    def two_calls():
        cut.append()
        app(cut.tag, cut.a_leaves, cut.a_off, cut.T, cut.max_new, cut.a_lv, one.d_add, one.d_aoff, one.T, one.max_new, two_leaves, two_off, two_lv,
            two_roots, None, None)
    row = _measure(one, a.reps)
    two_calls()
    torch.cuda.synchronize()
    same = bool(torch.equal(two_roots, one.a_roots)) and bool(torch.equal(two_off, one.a_off))
    t_one, t_two = C.alternate([one.append, two_calls], a.reps, C.event_ms)
    res["g"] = dict(row, trees=n_trees, swapped=int(cuts.sum()), one_call_ms=t_one, two_calls_ms=t_two, two_equal_one=same)
    say("G reorg: %d trees, %d leaves off and %d on: one call %.3f ms (%d digests)  resize then append %.3f ms  two/one %.2f  fresh build %.3f ms  "
        "build/one %.2f  identical %s, two calls equal one %s" % (n_trees, int(cuts.sum()), int(cuts.sum()), t_one, row["digests"], t_two, t_two / t_one,
                                                                 row["rebuild_ms"], row["rebuild_ms"] / t_one, row["identical"], same))
    del one, cut
    torch.cuda.empty_cache()
    for arity in (4, 2):
        rows = [r for r in res["a"] if r["arity"] == arity]
        lose = [r for r in rows if r["ratio"] < 1.0]
        say("arity %d: a fresh build is as quick from %s removed leaves of %d" % (arity, ("%d (1/%d of the tree)" % (lose[0]["removed"], rows[0]["leaves"] // lose[0]["removed"])) if lose else "none of the sweep", rows[0]["leaves"]))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
