#!/usr/bin/env python3
"""Leaf updates of a ragged forest applied in order, each with its witness (p252_merkle{4,2}_forest_ragged_update_sequential_device_into),
against what it replaces and what it cannot go below, timed in the same run:
 (a) the only other route to the same result: per update one p252_merkle{4,2}_forest_ragged_openings_device (k = 1) and one
     _forest_ragged_update_device (k = 1), timed as a loop over 256 updates and stated per update; the new call at k = 256 beside it;
 (b) p252_merkle{4,2}_path_ragged_device over k openings of the same depths: the k x depth digests every result inherently needs
     (each intermediate root is a different value) — a ratio, no threshold;
 (c) _forest_ragged_update_device on the same pairs where they are distinct: what the per-update witnesses cost over the update that
     hashes every dirty node once.

  python bench_tools/forest_sequential_bench.py [--reps 20] [--out profiles/forest_sequential.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket; the loop of (a) is one bracket around its 512 launches); the sides of a comparison alternate in the one process; the shader
clock is probed before and after.  Per arity, on one tree of 4^12 leaves (arity 2: 2^24): k = 1, 2^10, 2^16, 2^20 uniformly random
updates (pairs repeat as they fall), and the same k all on the first 16 leaves.  Then the mixed forest of forest_ragged_bench.py
(--trees trees, leaf counts log-uniform in [1, 4^7], seed 7, arity 4) with 2^16 updates, the tree drawn uniformly.  The order the call
takes is made once per workload, outside the brackets.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Forest
from testsupport import forestsequential as FS
from testsupport import treeshape as TS


def _measure(f, tid, lid, reps, loop=0):
    """f: a built Forest; the updates (numpy).  loop: the updates the existing route is timed over (0: not timed)"""
    import torch
    ctx, arity, k = f.ctx, f.arity, len(tid)
    dev = f.d.device
    D = int(TS.depth(f.max_leaves, arity))
    d_tid, d_lid = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(lid, np.uint64))
    d_order = C.dev(FS.stable_order(tid, lid))
    new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device=dev)
    old = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((k, max(D, 1), arity - 1, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((k, max(D, 1)), dtype=torch.uint8, device=dev)
    dep = torch.zeros(k, dtype=torch.uint8, device=dev)
    before, after, back = (torch.zeros((k, 4), dtype=torch.int64, device=dev) for _ in range(3))
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    hashed = torch.zeros(2, dtype=torch.int64, device=dev)
    seq = ctx.merkle4_forest_ragged_update_sequential_device if arity == 4 else ctx.merkle2_forest_ragged_update_sequential_device

    def run_seq():
        seq(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_lid, new, d_order, k, sib, pos, dep, after, d_old_leaves=old,
            d_roots_before=before, d_roots=f.roots, d_n_bad=bad[:1], d_n_hashed=hashed[:1])

    def run_path():  # (b): the digests alone, over the witnesses the call wrote
        ctx.merkle_path_ragged_device(f.tag, new, sib, pos, dep, D, back, k, arity=arity)
    pairs = np.unique(np.stack([np.asarray(tid, np.int64), np.asarray(lid, np.int64)]), axis=1)
    distinct = pairs.shape[1]
    u_tid, u_lid = C.dev(pairs[0].astype(np.uint32)), C.dev(pairs[1].astype(np.uint64))

    def run_update():  # (c): the deduplicating update on the distinct pairs
        ctx.merkle_forest_ragged_update_device(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, u_tid, u_lid, new, distinct, d_roots=f.roots,
                                               d_n_hashed=hashed[1:], arity=arity)
    hashed.zero_()
    run_seq(), run_update()
    torch.cuda.synchronize()
    digests, update_digests = int(hashed[0]), int(hashed[1])
    run_path()
    torch.cuda.synchronize()
    rehash_ok = bool(torch.equal(back, after))
    fns = [run_seq, run_path, run_update]
    if loop:
        o = tuple(torch.zeros_like(t[:1]) for t in (old, sib, pos, dep))
        ones = [(d_tid[i:i + 1], d_lid[i:i + 1], new[i:i + 1]) for i in range(loop)]

        def run_loop():  # (a): the existing route, one opening and one update per update
            for t1, l1, v1 in ones:
                ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, t1, l1, 1, out=o, arity=arity)
                ctx.merkle_forest_ragged_update_device(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, t1, l1, v1, 1, d_roots=f.roots, arity=arity)
        run_loop()
        fns.append(run_loop)
    ts = C.alternate(fns, reps, C.event_ms)
    r = {"k": k, "distinct": distinct, "depth": D, "bad": int(bad[0]), "digests": digests, "update_digests": update_digests, "rehash_ok": rehash_ok,
         "seq_ms": ts[0], "path_ms": ts[1], "seq_over_path": ts[0] / ts[1], "update_ms": ts[2], "seq_over_update": ts[0] / ts[2],
         "us_per_update": ts[0] / k * 1e3}
    if loop:
        r.update(loop=loop, loop_ms=ts[3], loop_us_per_update=ts[3] / loop * 1e3)
    return r


def _line(r):
    s = ("k = %d (%d distinct pairs, depth %d): the call %.3f ms = %.3f us an update, %d digests needed  (b) path_ragged over the same k openings %.3f ms: "
         "the call is x%.2f of it  (c) update_device on the distinct pairs %.3f ms (%d digests): the witnesses cost x%.2f  re-hash of (new leaf, opening) == "
         "roots_after: %s, bad %d" % (r["k"], r["distinct"], r["depth"], r["seq_ms"], r["us_per_update"], r["digests"], r["path_ms"], r["seq_over_path"],
                                      r["update_ms"], r["update_digests"], r["seq_over_update"], r["rehash_ok"], r["bad"]))
    if "loop" in r:
        s += ("  (a) the loop of openings (k = 1) + update (k = 1) over %d updates %.3f ms = %.1f us an update: the call is x%.1f ahead"
              % (r["loop"], r["loop_ms"], r["loop_us_per_update"], r["loop_us_per_update"] / r["us_per_update"]))
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_sequential.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, k up to 2^12, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "one_tree": []}
    say("python bench_tools/forest_sequential_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    rng = np.random.default_rng(a.seed)
    shapes = ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24))
    ks = [1, 1 << 8, 1 << 10, 1 << 12] if a.quick else [1, 1 << 8, 1 << 10, 1 << 16, 1 << 20]
    for arity, n in shapes:
        f = Forest(ctx, arity, [n], n)
        for spread, top in (("uniformly random leaves", n), ("all on the first 16 leaves", 16)):
            for k in ks:
                if k == 1 << 8 and top == 16:
                    continue  # (k = 256 is comparison (a)'s shape; once per tree)
                r = dict(_measure(f, np.zeros(k, np.uint32), rng.integers(0, top, size=k), a.reps, loop=256 if k == 1 << 8 else 0), arity=arity, tree=n,
                         spread=spread)
                res["one_tree"].append(r)
                say("arity %d, one tree of %d leaves, %s: %s" % (arity, n, spread, _line(r)))
        del f
        torch.cuda.empty_cache()
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    f = Forest(ctx, 4, sizes, top)
    k = 1 << 12 if a.quick else 1 << 16
    tid = rng.integers(0, n_trees, size=k)
    r = dict(_measure(f, tid, (rng.random(k) * sizes[tid]).astype(np.int64), a.reps), arity=4, trees=n_trees)
    res["mixed"] = r
    say("arity 4, %d trees (log-uniform 1..4^7, %d leaves), the tree drawn uniformly: %s" % (n_trees, int(sizes.sum()), _line(r)))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    say("not measured: the device sort that makes d_order (outside every bracket), k above 2^20, more than one stream, other trees' depths")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
