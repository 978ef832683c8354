#!/usr/bin/env python3
"""Consistency proofs of a ragged forest (p252_merkle{4,2}_forest_ragged_consistency_device_into: the extraction, no digest;
_forest_consistency_verify_device_into: two chains over one opening) against the calls they are built beside, timed in the same run:
the extraction against p252_merkle{4,2}_forest_ragged_openings_device of the same (tree, leaf) pairs, the verification against
p252_merkle{4,2}_forest_ragged_verify_device on the same openings (the new-root half alone), and against the only other route to the
same statement — replaying the appended leaves through p252_merkle{4,2}_forest_frontier_append_device_into.

  python bench_tools/forest_consistency_bench.py [--reps 20] [--out profiles/forest_consistency.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket); the sides of a comparison alternate in the one process; the shader clock is probed before and after.
A: one tree of 4^12 leaves (arity 4) with 2^20 random old counts.  B: one tree of 2^24 leaves (arity 2) with 2^20 random old counts.
C: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7), one proof per tree.
Replay: the trees of A and B at 1, 2^16 and 2^20 leaves fewer, and those leaves appended to the frontier state (one old root checked per
replay; a consistency proof checks one per lane).
Beside the times: the digests the verification computes against the depth(m) per proof of the older call (the bound is twice that), and
the spread (max / min over the --reps launches) of the older call, which is what a ratio above the bound has to be read against.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Case, Forest
from testsupport import treeshape as TS


def _times(fns, reps):
    """per callable the list of --reps event times (ms), the callables run in turn"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(C.event_ms(fn))
    return ts


def _measure(f, tid, old, reps):
    """f: a built Forest; (tid, old): the proofs.  -> the times and counts of one workload"""
    import torch
    ctx, arity, k = f.ctx, f.arity, len(tid)
    dev = f.d.device
    d_tid, d_old = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(old, np.uint64))
    D = int(TS.depth(f.max_leaves, arity))
    newc = torch.zeros(k, dtype=torch.int64, device=dev)
    lv = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((k, D, arity - 1, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((k, D), dtype=torch.uint8, device=dev)
    dep = torch.zeros(k, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    o_out = tuple(torch.zeros_like(t) for t in (lv, sib, pos, dep))
    extract = ctx.merkle4_forest_ragged_consistency_device if arity == 4 else ctx.merkle2_forest_ragged_consistency_device
    verify = ctx.merkle4_forest_consistency_verify_device if arity == 4 else ctx.merkle2_forest_consistency_verify_device

    def run_extract():
        extract(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_old, k, newc, lv, sib, pos, dep, bad)

    def run_openings():
        ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_old, k, out=o_out, arity=arity)
    run_extract(), run_openings()
    torch.cuda.synchronize()
    grown = (newc > d_old)
    same_bytes = all(bool(torch.equal(a[grown], b[grown])) for a, b in zip((lv, sib, pos, dep), o_out))
    # the claims: the old roots are what the left siblings re-hash to (the tests compare those with the oracle); the new ones the forest's
    ok = torch.zeros(k, dtype=torch.uint8, device=dev)
    ok2 = torch.zeros(k, dtype=torch.uint8, device=dev)
    old_roots, new_out = torch.zeros((k, 4), dtype=torch.int64, device=dev), torch.zeros((k, 4), dtype=torch.int64, device=dev)
    hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    new_roots = f.roots[d_tid.to(torch.int64)].contiguous()
    verify(f.tag, d_old, new_roots, newc, new_roots, lv, sib, pos, dep, D, k, ok, None, 0, old_roots, new_out, hashed)
    torch.cuda.synchronize()
    old_roots = torch.where(grown.view(k, 1), old_roots, new_roots)  # (an unchanged tree: old root == new root)
    new_same = bool(torch.equal(new_out[grown], new_roots[grown]))

    def run_verify():
        verify(f.tag, d_old, old_roots, newc, new_roots, lv, sib, pos, dep, D, k, ok)

    def run_plain():
        ctx.merkle_forest_ragged_verify_device(f.tag, lv, sib, pos, dep, D, d_tid, f.roots, f.n_trees, ok2, k, arity=arity)
    run_verify(), run_plain()
    torch.cuda.synchronize()
    n_ok, n_plain_ok = int(ok.sum()), int(ok2[grown].sum())
    t_ext, t_open, t_ver, t_plain = _times([run_extract, run_openings, run_verify, run_plain], reps)
    med = lambda t: float(np.median(t))  # noqa: E731
    depth_sum = int(dep[grown].to(torch.int64).sum())
    return {"proofs": k, "grown": int(grown.sum()), "bad": int((dep == 0xFF).sum()), "extract_ms": med(t_ext), "openings_ms": med(t_open),
            "extract_over_openings": med(t_ext) / med(t_open), "verify_ms": med(t_ver), "plain_verify_ms": med(t_plain),
            "verify_over_plain": med(t_ver) / med(t_plain), "plain_spread": max(t_plain) / min(t_plain), "verify_spread": max(t_ver) / min(t_ver),
            "digests": int(hashed), "digests_plain": depth_sum, "digests_over_plain": int(hashed) / max(depth_sum, 1),
            "extraction_identical": same_bytes, "new_roots_identical": new_same, "ok": n_ok, "plain_ok": n_plain_ok}


FORMAT = ("%d proofs (%d of grown trees): extraction %.3f ms against openings %.3f ms (%.2f, bytes identical %s)  verification %.3f ms "
          "against forest_ragged_verify %.3f ms: ratio %.2f (digests %d against %d: %.2f; spread of the older call %.2f, of this one %.2f)  "
          "ok %d of %d, older call ok %d of %d, new roots identical %s")


def _line(r):
    return FORMAT % (r["proofs"], r["grown"], r["extract_ms"], r["openings_ms"], r["extract_over_openings"], r["extraction_identical"], r["verify_ms"],
                     r["plain_verify_ms"], r["verify_over_plain"], r["digests"], r["digests_plain"], r["digests_over_plain"], r["plain_spread"],
                     r["verify_spread"], r["ok"], r["proofs"], r["plain_ok"], r["grown"], r["new_roots_identical"])


def _replay(ctx, arity, n_new, x, reps):
    """x leaves appended to the frontier state of a tree of n_new - x leaves: the replay that checks ONE old root"""
    import torch
    from poseidon252_amd import merkle as M
    case = Case(ctx, arity, [n_new - x], [x])
    base, _ = M.ForestFrontier.from_forest(ctx, case.d, case.d_off, 1, case.max_old, case.lv, case.roots_old, max_leaves=case.max_new, arity=arity)
    work = M.ForestFrontier(ctx, 1, case.max_new, arity, device=case.d.device)
    call = ctx.merkle4_forest_frontier_append_device if arity == 4 else ctx.merkle2_forest_frontier_append_device

    def restored(fn):
        work.counts.copy_(base.counts), work.frontier.copy_(base.frontier), work.roots.copy_(base.roots)
        return C.event_ms(fn)
    run = lambda: call(case.tag, work.counts, work.frontier, work.roots, 1, case.max_new, case.d_add, case.d_aoff, None, None)  # noqa: E731
    restored(run)
    ms = float(np.median([restored(run) for _ in range(reps)]))
    torch.cuda.synchronize()
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_consistency.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2^14 proofs, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "one_tree": [], "replay": []}
    say("python bench_tools/forest_consistency_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    rng = np.random.default_rng(a.seed)
    k = 1 << 14 if a.quick else 1 << 20
    shapes = ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24))

    # ---- A, B: one tree, many old counts ----
    for name, (arity, n) in zip("AB", shapes):
        f = Forest(ctx, arity, [n], n)
        old = rng.integers(1, n, k)  # 1 <= n_old < n
        r = dict(_measure(f, np.zeros(k, np.uint32), old, a.reps), arity=arity, leaves=n)
        res["one_tree"].append(r)
        say("%s arity %d, one tree of %d leaves: %s" % (name, arity, n, _line(r)))
        del f
        torch.cuda.empty_cache()

    # ---- C: the mixed forest, one proof per tree ----
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    f = Forest(ctx, 4, sizes, top)
    old = np.maximum((rng.random(n_trees) * sizes).astype(np.int64), 1)  # 1 <= n_old <= n_t (a one-leaf tree: unchanged)
    r = dict(_measure(f, np.arange(n_trees, dtype=np.uint32), old, a.reps), arity=4, trees=n_trees, leaves=int(sizes.sum()))
    res["mixed"] = r
    say("C arity 4, %d trees (log-uniform 1..4^7, %d leaves), one proof per tree: %s" % (n_trees, r["leaves"], _line(r)))
    del f
    torch.cuda.empty_cache()

    # ---- the replay ----
    for arity, n in shapes:
        for x in ([1, 1 << 6, 1 << 10] if a.quick else [1, 1 << 16, 1 << 20]):
            ms = _replay(ctx, arity, n, x, a.reps)
            one = next(t for t in res["one_tree"] if t["arity"] == arity)
            per_proof_us = one["verify_ms"] / one["proofs"] * 1e3
            res["replay"].append({"arity": arity, "leaves": n, "appended": x, "replay_ms": ms, "verify_us_per_proof": per_proof_us})
            say("replay arity %d, %d leaves, m - n = %d: frontier append %.3f ms for ONE old root; the verification above takes %.3f us per proof "
                "(%.0f proofs in the time of one replay)" % (arity, n, x, ms, per_proof_us, ms * 1e3 / per_proof_us))
            torch.cuda.empty_cache()
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
