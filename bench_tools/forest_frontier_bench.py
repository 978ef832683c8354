#!/usr/bin/env python3
"""Leaves appended to a forest kept only as its frontiers (p252_merkle{4,2}_forest_frontier_append_device_into: O(depth) state per
tree, updated in place) against the same appends through the stored forest (p252_merkle{4,2}_forest_ragged_append_device_into) and
against a fresh p252_merkle{4,2}_forest_ragged_device build of the grown forest, timed in the same run.

  python bench_tools/forest_frontier_bench.py [--reps 20] [--out profiles/forest_frontier.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock
inside the bracket); the three sides alternate in the one process; the frontier call works in place, so its state is put back to the
extracted one before every launch, outside the bracket; the roots of the two appends are compared byte for byte; the shader clock is
probed before and after.
A, one tree: 4^12 leaves (arity 4) and 2^24 leaves (arity 2) plus 2^0, 2^16, 2^20 appended leaves.
B, many trees: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7) with 1 to 16
leaves appended to EVERY tree.  C: the same with leaves appended to 1 % of the trees.
Beside the times: the bytes of the frontier state (counts, rows, roots) and of the stored forest (leaves, levels, offsets, roots), and
the launches of each call as the launchers make them.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Case
from testsupport import treeshape as TS

FRONTIER_FIXED_LAUNCHES = 11  # csrc/forest_frontier.hip: sizes, the sum rule's 3, refused, the dirty lists' 4, records, finish; plus one digest launch per level
APPEND_FIXED_LAUNCHES = 30    # csrc/forest_append.hip, as its header comment counts them; plus one digest launch per level


class Frontier:
    """the frontier state of a Case's old forest, and the in-place append of the Case's leaves to it"""

    def __init__(self, case):
        import torch
        from poseidon252_amd import merkle as M
        self.case = case
        self.base, _ = M.ForestFrontier.from_forest(case.ctx, case.d, case.d_off, case.T, case.max_old, case.lv, case.roots_old, max_leaves=case.max_new,
                                                    arity=case.arity)
        self.work = M.ForestFrontier(case.ctx, case.T, case.max_new, case.arity, device=case.d.device)
        self.hashed = torch.zeros(1, dtype=torch.int64, device=case.d.device)
        self.call = case.ctx.merkle4_forest_frontier_append_device if case.arity == 4 else case.ctx.merkle2_forest_frontier_append_device

    def restore(self):
        self.work.counts.copy_(self.base.counts), self.work.frontier.copy_(self.base.frontier), self.work.roots.copy_(self.base.roots)

    def append(self, count=False):
        c, w = self.case, self.work
        self.call(c.tag, w.counts, w.frontier, w.roots, c.T, c.max_new, c.d_add, c.d_aoff, None, self.hashed if count else None)

    def state_bytes(self):
        w = self.work
        return sum(t.numel() * t.element_size() for t in (w.counts, w.frontier, w.roots))


def _restored_event_ms(front):
    def timer(fn):
        front.restore()
        return C.event_ms(fn)
    return timer


def _measure(case, reps):
    import torch
    front = Frontier(case)
    front.restore()
    front.hashed.zero_()
    front.append(count=True)
    case.append(count=True)
    case.rebuild()
    torch.cuda.synchronize()
    same = bool(torch.equal(front.work.roots, case.a_roots)) and bool(torch.equal(case.a_roots, case.b_roots))
    same = same and bool(torch.equal(front.work.counts, case.a_off[1:] - case.a_off[:-1]))
    t_front, t_app, t_build = C.alternate([front.append, case.append, case.rebuild], reps, _restored_event_ms(front))
    torch.cuda.synchronize()
    stored = sum(t.numel() * t.element_size() for t in (case.a_leaves, case.a_lv, case.a_off, case.a_roots))
    depth = int(TS.depth(case.max_new, case.arity))
    return {"frontier_ms": t_front, "append_ms": t_app, "rebuild_ms": t_build, "frontier_over_append": t_front / t_app,
            "digests": int(front.hashed), "digests_append": int(case.hashed), "roots_identical": same, "state_bytes": front.state_bytes(),
            "stored_bytes": stored, "launches_frontier": FRONTIER_FIXED_LAUNCHES + depth, "launches_append": APPEND_FIXED_LAUNCHES + depth}


FORMAT = ("frontier append %.3f ms (%d digests, %d launches)  stored append %.3f ms (%d digests, about %d launches)  fresh build %.3f ms  "
          "frontier/append %.2f  build/frontier %.1f  state %d bytes against %d stored (1/%.0f)  roots identical %s")


def _line(r):
    return FORMAT % (r["frontier_ms"], r["digests"], r["launches_frontier"], r["append_ms"], r["digests_append"], r["launches_append"], r["rebuild_ms"],
                     r["frontier_over_append"], r["rebuild_ms"] / r["frontier_ms"], r["state_bytes"], r["stored_bytes"],
                     r["stored_bytes"] / max(r["state_bytes"], 1), r["roots_identical"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_frontier.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "a": []}
    say("python bench_tools/forest_frontier_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))

    # ---- A: one tree ----
    for arity, n in ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24)):
        for m in ([1, 1 << 6, 1 << 10] if a.quick else [1, 1 << 16, 1 << 20]):
            c = Case(ctx, arity, [n], [m])
            r = dict(_measure(c, a.reps), arity=arity, leaves=n, appended=m)
            res["a"].append(r)
            say("A arity %d, %d leaves + %d: %s" % (arity, n, m, _line(r)))
            del c
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
        say("%s: %d trees (log-uniform 1..4^7, %d leaves), %d leaves appended to %d trees: %s"
            % (name.upper(), n_trees, r["leaves"], r["appended"], r["trees_appended_to"], _line(r)))
        del c
        torch.cuda.empty_cache()
    # the yardstick: where both calls compute the same digests (>= 2^16 appended leaves) this one relocates nothing
    wide = [r for r in res["a"] if r["appended"] >= 1 << 16]
    behind = [r for r in wide if r["frontier_over_append"] > 1.0]
    say("rows with >= 2^16 appended leaves: %d, frontier/append %s; behind the stored append on %d of them%s"
        % (len(wide), ", ".join("%.2f" % r["frontier_over_append"] for r in wide) or "-", len(behind),
           "".join(" (arity %d + %d: %.3f against %.3f ms)" % (r["arity"], r["appended"], r["frontier_ms"], r["append_ms"]) for r in behind)))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
