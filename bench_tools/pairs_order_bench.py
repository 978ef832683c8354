#!/usr/bin/env python3
"""The order and the distinct (tree id, leaf id) pairs made by the library on the device (p252_pairs_order_device_into,
p252_pairs_unique_device_into) against the route merkle.py takes today and against what no sort can go below, timed in the same run:
 (a) the baseline: two stable torch.sort calls (by leaf, then by tree) for the order; torch.unique on the packed 64-bit key
     (tree << 32 | leaf) for the distinct pairs — not timed where a key does not pack into 64 bits;
 (b) the floor: one device-to-device copy of the k 16-byte records, times the passes that ran (testsupport/pairsmodel.py says which);
 (c) end to end: p252_merkle4_forest_ragged_update_sequential_device_into with the order made by each route inside the bracket, and
     the update alone.

  python bench_tools/pairs_order_bench.py [--reps 20] [--out profiles/pairs_order.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket); the sides of a comparison alternate in the one process; the shader clock is probed before and after.  Rows at k = 2^10,
2^16, 2^20: uniformly random pairs of one tree of 4^12 leaves; the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts
log-uniform in [1, 4^7], seed 7), the tree drawn uniformly; all k on the first 16 leaves of one tree; random full-width 96-bit keys,
the 12-pass worst case.  Every result is compared with the numpy model before it is timed.
Prints one line per row, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Forest
from testsupport import pairsmodel as PM
from testsupport import treeshape as TS


def _measure(ctx, t, j, reps):
    import torch
    k = j.size
    d_t, d_j = C.dev(t), C.dev(j)
    dev = d_j.device
    order = torch.zeros(k, dtype=torch.int32, device=dev)
    t_out, idx_out, first = (torch.zeros(k, dtype=torch.int32, device=dev) for _ in range(3))
    j_out = torch.zeros(k, dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    recs, recs2 = (torch.zeros((k, 2), dtype=torch.int64, device=dev) for _ in range(2))
    packs = int(t.max()) < 1 << 31 and int(j.max()) < 1 << 32
    t64, j64 = d_t.to(torch.int64) & 0xFFFFFFFF, d_j

    def lib_order():
        ctx.pairs_order_device(d_t, d_j, k, order)

    def lib_unique():
        ctx.pairs_unique_device(d_t, d_j, k, n, d_tree_ids_out=t_out, d_leaf_ids_out=j_out, d_indices_out=idx_out, d_first=first)

    def torch_order():
        by_leaf = torch.sort(j64, stable=True).indices
        return by_leaf[torch.sort(t64[by_leaf], stable=True).indices].to(torch.int32)

    def torch_unique():
        return torch.unique((t64 << 32) | j64)

    def copy():
        recs2.copy_(recs)
    lib_order(), lib_unique()
    torch.cuda.synchronize()
    want = PM.order(t, j)
    wt, wj, wf = PM.unique(t, j)
    m = int(n)
    exact = bool(np.array_equal(order.cpu().numpy().view(np.uint32), want) and m == wt.size and
                 np.array_equal(t_out[:m].cpu().numpy().view(np.uint32), wt) and np.array_equal(j_out[:m].cpu().numpy().view(np.uint64), wj) and
                 np.array_equal(first[:m].cpu().numpy().view(np.uint32), wf))
    passes = len(PM.varying_passes(t, j))
    fns = [lib_order, lib_unique, torch_order, copy] + ([torch_unique] if packs else [])
    for fn in fns:
        fn()
    ts = C.alternate(fns, reps, C.event_ms)
    r = {"k": int(k), "distinct": m, "passes": passes, "exact": exact, "order_ms": ts[0], "unique_ms": ts[1], "torch_order_ms": ts[2],
         "order_over_torch": ts[0] / ts[2], "copy_ms": ts[3], "floor_ms": ts[3] * passes, "order_over_floor": ts[0] / (ts[3] * passes)}
    if packs:
        r.update(torch_unique_ms=ts[4], unique_over_torch=ts[1] / ts[4])
    return r


def _line(r):
    s = ("k = %d (%d distinct, %d of 12 passes run): the order %.3f ms  (a) two stable torch.sort %.3f ms: the call is x%.2f of it  (b) %d copies of "
         "the records %.3f ms: the call is x%.1f of that floor  the distinct pairs %.3f ms"
         % (r["k"], r["distinct"], r["passes"], r["order_ms"], r["torch_order_ms"], r["order_over_torch"], r["passes"], r["floor_ms"],
            r["order_over_floor"], r["unique_ms"]))
    s += ("  (a) torch.unique on the packed key %.3f ms: the call is x%.2f of it" % (r["torch_unique_ms"], r["unique_over_torch"])
          if "torch_unique_ms" in r else "  (a) torch.unique: a 96-bit key does not pack into 64 bits")
    return s + "  equal to the numpy model: %s" % r["exact"]


def _end_to_end(f, tid, lid, reps):
    """(c): the sequential update of the forest f with the order made inside the bracket by the library, by torch, and not at all"""
    import torch
    ctx, k = f.ctx, len(tid)
    dev = f.d.device
    D = int(TS.depth(f.max_leaves, 4))
    d_t, d_j = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(lid, np.uint64))
    t64 = d_t.to(torch.int64)
    order = torch.zeros(k, dtype=torch.int32, device=dev)
    new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((k, max(D, 1), 3, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((k, max(D, 1)), dtype=torch.uint8, device=dev)
    dep = torch.zeros(k, dtype=torch.uint8, device=dev)
    after = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def update(o):
        ctx.merkle4_forest_ragged_update_sequential_device(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_t, d_j, new, o, k, sib, pos, dep, after,
                                                           d_roots=f.roots, d_n_bad=bad)

    def with_lib():
        ctx.pairs_order_device(d_t, d_j, k, order)
        update(order)

    def with_torch():
        by_leaf = torch.sort(d_j, stable=True).indices
        update(by_leaf[torch.sort(t64[by_leaf], stable=True).indices].to(torch.int32))

    def alone():
        update(order)
    with_lib(), with_torch(), alone()
    torch.cuda.synchronize()
    ts = C.alternate([with_lib, with_torch, alone], reps, C.event_ms)
    return {"k": int(k), "bad": int(bad), "lib_ms": ts[0], "torch_ms": ts[1], "update_alone_ms": ts[2]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_order.txt"), help="where the rows are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (a 4^8-leaf tree, k up to 2^12, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "rows": [], "end_to_end": []}
    say("python bench_tools/pairs_order_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    rng = np.random.default_rng(a.seed)
    n = 4 ** 8 if a.quick else 4 ** 12
    ks = [1 << 8, 1 << 10, 1 << 12] if a.quick else [1 << 10, 1 << 16, 1 << 20]
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    for k in ks:
        tid = rng.integers(0, n_trees, size=k)
        rows = (("one tree of %d leaves, uniformly random leaves" % n, np.zeros(k, np.uint32), rng.integers(0, n, size=k).astype(np.uint64)),
                ("%d trees (log-uniform 1..4^7), the tree drawn uniformly" % n_trees, tid.astype(np.uint32), (rng.random(k) * sizes[tid]).astype(np.uint64)),
                ("one tree, all on the first 16 leaves", np.zeros(k, np.uint32), rng.integers(0, 16, size=k).astype(np.uint64)),
                ("random full-width 96-bit keys", rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32),
                 rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)))
        for what, t, j in rows:
            r = dict(_measure(ctx, t, j, a.reps), keys=what)
            res["rows"].append(r)
            say("%s: %s" % (what, _line(r)))
    f = Forest(ctx, 4, [n], n)
    for k in ks:
        r = _end_to_end(f, np.zeros(k, np.uint32), rng.integers(0, n, size=k), a.reps)
        res["end_to_end"].append(r)
        say("(c) update_sequential_device, one tree of %d leaves, k = %d uniformly random updates: with the library's order inside the bracket %.3f ms, "
            "with torch's %.3f ms, the update alone %.3f ms (bad %d)" % (n, k, r["lib_ms"], r["torch_ms"], r["update_alone_ms"], r["bad"]))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    say("not measured: k above 2^20, more than one stream, the calls inside a captured graph, host-side time of the torch route's allocations")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
