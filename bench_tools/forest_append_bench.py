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
Prints one line per workload, writes them to --out, and prints a JSON summary last.

The module also holds forest_append_model, the numpy model of the call that the tests compare it with."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _depth(n, arity):
    d = 0
    while n > 1:
        n = (n + arity - 1) // arity
        d += 1
    return d


def level_widths(n, arity):
    """nodes of levels 1, 2, .. of a tree of n leaves (none for n <= 1)"""
    w = []
    while n > 1:
        n = (n + arity - 1) // arity
        w.append(n)
    return w


def good_leaf_counts(offsets, n_leaves, max_leaves):
    """the build's validation of a forest (k_fr_prep and the sum rule): n_t, or 0 for a bad tree"""
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    out, run = [], 0
    for t in range(len(off) - 1):
        lo, hi = off[t], off[t + 1]
        n = hi - lo
        n = n if (hi >= lo and 1 <= n <= max_leaves and hi <= n_leaves) else 0
        if run > n_leaves or n > n_leaves - run:
            run, n = run + n, 0
        else:
            run += n
        out.append(n)
    return out


def forest_append_model(offsets, n_leaves, max_leaves, add_offsets, n_add, max_leaves_new, arity):
    """What p252_merkle{4,2}_forest_ragged_append_device_into does to a forest (offsets: n_trees + 1, or empty for no old forest) given
    add_offsets (n_trees_new + 1).  Returns a dict:
      n_old, m, refused   per tree of the new forest: the old leaf count (the build's validation), the accepted append, its refusal
      offsets_new         n_trees_new + 1
      leaf_src            per new leaf: its index in the old leaves, or -1 - (its index in d_add)
      lo_new, lo_old      block starts of the tree-major levels, n_trees_new + 1 / n_trees + 1
      node_src            per used slot of the new levels: the slot of the old levels it is moved from, or -1 (dirty: hashed)
      node_id             per used slot: (tree, level, index)
      dirty               {level: [(tree, index), ..]} in the order of the call's lists
      n_hashed, n_bad"""
    off = [int(x) for x in np.asarray(offsets).reshape(-1)]
    aoff = [int(x) for x in np.asarray(add_offsets).reshape(-1)]
    T = len(aoff) - 1
    old = good_leaf_counts(off, n_leaves, max_leaves) if len(off) > 1 else []
    n_old = [old[t] if t < len(old) else 0 for t in range(T)]
    m, refused, run = [], [], 0
    for t in range(T):
        lo, hi = aoff[t], aoff[t + 1]
        mt = hi - lo
        ok = hi >= lo and hi <= n_add and n_old[t] + mt <= max_leaves_new
        mt = mt if ok else 0
        if ok and mt and (run > n_add or mt > n_add - run):  # the sum rule: overlapping ranges behind decreasing offsets
            ok = False
        run += mt
        m.append(mt if ok else 0)
        refused.append(not ok)
    n_new = [a + b for a, b in zip(n_old, m)]
    offsets_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(n_new, out=offsets_new[1:])
    leaf_src = np.empty(int(offsets_new[-1]), dtype=np.int64)
    for t in range(T):
        at = int(offsets_new[t])
        if n_old[t]:
            leaf_src[at:at + n_old[t]] = off[t] + np.arange(n_old[t])
        if m[t]:
            leaf_src[at + n_old[t]:at + n_new[t]] = -1 - (aoff[t] + np.arange(m[t]))
    lo_old = np.zeros(len(old) + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in old], out=lo_old[1:])
    lo_new = np.zeros(T + 1, dtype=np.int64)
    np.cumsum([sum(level_widths(n, arity)) for n in n_new], out=lo_new[1:])
    node_src = np.full(int(lo_new[-1]), -1, dtype=np.int64)
    node_id = []
    dirty, n_hashed = {}, 0
    for t in range(T):
        w_new, w_old = level_widths(n_new[t], arity), level_widths(n_old[t], arity)
        start_new, start_old = int(lo_new[t]), int(lo_old[t]) if t < len(old) else 0
        for l, w in enumerate(w_new, 1):
            clean = w if m[t] == 0 else n_old[t] // arity ** l
            node_src[start_new:start_new + clean] = start_old + np.arange(clean)
            node_id += [(t, l, j) for j in range(w)]
            if w > clean:
                dirty.setdefault(l, []).extend((t, j) for j in range(clean, w))
                n_hashed += w - clean
            start_new += w
            if l <= len(w_old):
                start_old += w_old[l - 1]
    n_bad = sum(1 for t in range(T) if refused[t] or n_new[t] == 0)
    return {"n_old": n_old, "m": m, "refused": refused, "n_new": n_new, "offsets_new": offsets_new, "leaf_src": leaf_src, "lo_new": lo_new,
            "lo_old": lo_old, "node_src": node_src, "node_id": node_id, "dirty": dirty, "n_hashed": n_hashed, "n_bad": n_bad}


def model_leaves(model, leaves, add):
    """the new forest's leaves (numpy (n, 4)) from the old ones and d_add"""
    src = model["leaf_src"]
    leaves, add = np.asarray(leaves).reshape(-1, 4), np.asarray(add).reshape(-1, 4)
    out = np.empty((src.size, 4), dtype=leaves.dtype if leaves.size else add.dtype)
    old = src >= 0
    out[old] = leaves[src[old]]
    out[~old] = add[-1 - src[~old]]
    return out


# ---------------------------------------------------------------------------------------------
# the measurement
# ---------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a
    return torch.from_numpy(a).to("cuda:0")


def _event_ms(fn):
    """one launch of fn between two device events on the current stream"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(_event_ms(fn))
    return [float(np.median(t)) for t in ts]


def _clock_mhz(ctx):
    import torch
    try:
        t = ctx.clock_probe(spin_us=1000)
        torch.cuda.synchronize()
        return round(ctx.clock_probe_result(t)["shader_ghz"] * 1e3, 1)
    except Exception:  # (a measurement aid only)
        return None


class Case:
    """an old forest built on the device, an append to it, and the buffers of the appended and of the freshly built new forest"""

    def __init__(self, ctx, arity, sizes, adds):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.arity = ctx, arity
        sizes, adds = np.asarray(sizes, dtype=np.int64), np.asarray(adds, dtype=np.int64)
        self.T, self.n_leaves, self.n_add = len(sizes), int(sizes.sum()), int(adds.sum())
        self.max_old, self.max_new = int(sizes.max()), int((sizes + adds).max())
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        dev = torch.device("cuda:0")
        off = np.zeros(self.T + 1, dtype=np.int64)
        np.cumsum(sizes, out=off[1:])
        aoff = np.zeros(self.T + 1, dtype=np.int64)
        np.cumsum(adds, out=aoff[1:])
        self.d_off, self.d_aoff = _dev(off), _dev(aoff)
        self.d = torch.randint(0, 1 << 60, (self.n_leaves, 4), dtype=torch.int64, device=dev)
        self.d_add = torch.randint(0, 1 << 60, (self.n_add, 4), dtype=torch.int64, device=dev) if self.n_add else None
        cap = lambda n, mx: n // (arity - 1) + self.T * _depth(mx, arity)  # noqa: E731
        self.lv = torch.empty((cap(self.n_leaves, self.max_old), 4), dtype=torch.int64, device=dev)
        self.roots_old = torch.empty((self.T, 4), dtype=torch.int64, device=dev)
        ctx.merkle_forest_ragged_device(self.tag, self.d, self.d_off, self.T, self.max_old, self.roots_old, self.lv, arity=arity)
        total = self.n_leaves + self.n_add
        new = lambda: (torch.zeros((total, 4), dtype=torch.int64, device=dev), torch.zeros((cap(total, self.max_new), 4), dtype=torch.int64, device=dev),  # noqa: E731
                       torch.zeros((self.T, 4), dtype=torch.int64, device=dev))
        self.a_leaves, self.a_lv, self.a_roots = new()
        self.b_leaves, self.b_lv, self.b_roots = new()
        self.a_off = torch.zeros(self.T + 1, dtype=torch.int64, device=dev)
        self.hashed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.call = ctx.merkle4_forest_ragged_append_device if arity == 4 else ctx.merkle2_forest_ragged_append_device
        self.bytes_moved = None

    def append(self, count=False):
        self.call(self.tag, self.d, self.d_off, self.T, self.max_old, self.lv, self.d_add, self.d_aoff, self.T, self.max_new, self.a_leaves, self.a_off,
                  self.a_lv, self.a_roots, None, self.hashed if count else None)

    def rebuild(self):
        """the fresh build of the new forest, from the append's own leaves and offsets"""
        self.ctx.merkle_forest_ragged_device(self.tag, self.a_leaves, self.a_off, self.T, self.max_new, self.b_roots, self.b_lv, arity=self.arity)

    def identical(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.equal(self.a_roots, self.b_roots)) and bool(torch.equal(self.a_lv, self.b_lv))


def _measure(case, reps):
    import torch
    case.append(count=True)
    case.rebuild()
    same = case.identical()
    hashed = int(case.hashed)
    t_app, t_build = _alternate([case.append, case.rebuild], reps)
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
    res = {"reps": a.reps, "clock_mhz_before": _clock_mhz(ctx), "a": [], "r": []}
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
        t_move, t_copy = _alternate([c.append, lambda: dst.copy_(src)], a.reps)
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
    res["clock_mhz_after"] = _clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
