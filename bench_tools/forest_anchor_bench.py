#!/usr/bin/env python3
"""Roots and openings of a grown forest against its earlier roots (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into) against
the calls it is built beside, timed in the same run: p252_merkle{4,2}_forest_ragged_openings_device of the same (tree, leaf) pairs on the
current forest (the pure-gather floor: nothing hashed, nothing cut off), the only other route to the same bytes — one
p252_merkle{4,2}_forest_ragged_resize_device_into (keep = c) into a second copy of the forest, then the openings call on the copy — and,
for the roots alone (k = 0), consistency extraction plus verification of the same (tree, count) pairs.

  python bench_tools/forest_anchor_bench.py [--reps 20] [--out profiles/forest_anchor.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket); the sides of a comparison alternate in the one process; the shader clock is probed before and after.
A: one tree of 4^12 leaves (arity 4) with 1, 2^10 and 2^20 anchors at random counts, each with 2^20 openings of random leaves below
their anchor's count.  B: one tree of 2^24 leaves (arity 2) likewise.  With 2^20 anchors also the digests per second of the anchors'
chains against p252_merkle{4,2}_path_ragged_device on 2^20 openings of the same depth, the project's own rate for per-lane chains.
C: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7), one anchor per tree 1 .. 16
leaves back, 1 .. 16 openings per anchor; against the plain openings call, and against resize(keep) plus openings with the extra device
memory that route needs.
D: 2^16 anchors of one 4^12-leaf tree, counts of mixed chain lengths against counts that all have the longest chain: the digests run
level by level over all anchors, so what mixed lengths cost is idle digests, not divergence.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Forest
from testsupport import forestanchor as FA
from testsupport import treeshape as TS


def _times(fns, reps):
    """per callable the list of --reps event times (ms), the callables run in turn"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(C.event_ms(fn))
    return ts


def med(t):
    return float(np.median(t))


class Anchors:
    """the buffers of one workload: m anchors (tree, count), k openings (anchor, leaf) of the built Forest f"""

    def __init__(self, f, a_tree, a_count, o_anchor, o_leaf):
        import torch
        self.f, self.m, self.k = f, len(a_tree), len(o_anchor)
        dev = f.d.device
        self.D = int(TS.depth(f.max_leaves, f.arity))
        self.a_tree_np, self.a_count_np = np.asarray(a_tree, np.int64), np.asarray(a_count, np.int64)
        self.d_at, self.d_ac = C.dev(np.asarray(a_tree, np.uint32)), C.dev(np.asarray(a_count, np.uint64))
        self.d_oa, self.d_ol = C.dev(np.asarray(o_anchor, np.uint32)), C.dev(np.asarray(o_leaf, np.uint64))
        self.d_ot = C.dev(self.a_tree_np[np.asarray(o_anchor, np.int64)].astype(np.uint32)) if self.k else None  # the openings' trees
        m, k, D, per = self.m, self.k, self.D, f.arity - 1
        self.roots = torch.zeros((m, 4), dtype=torch.int64, device=dev)
        self.depths = torch.zeros(m, dtype=torch.uint8, device=dev)
        mk = lambda: (torch.zeros((k, 4), dtype=torch.int64, device=dev), torch.zeros((k, D, per, 4), dtype=torch.int64, device=dev),  # noqa: E731
                      torch.zeros((k, D), dtype=torch.uint8, device=dev), torch.zeros(k, dtype=torch.uint8, device=dev))
        self.out, self.plain = mk(), mk()
        self.bad = torch.zeros(2, dtype=torch.int32, device=dev)
        self.hashed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.call = f.ctx.merkle4_forest_ragged_anchor_openings_device if f.arity == 4 else f.ctx.merkle2_forest_ragged_anchor_openings_device

    def run(self, count=False):
        f, o = self.f, self.out
        self.call(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, self.d_at, self.d_ac, self.m, self.d_oa, self.d_ol, self.k, self.roots, self.depths,
                  o[0], o[1], o[2], o[3], self.bad[:1] if count else None, self.bad[1:] if count else None, self.hashed if count else None)

    def run_roots(self):
        f = self.f
        self.call(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, self.d_at, self.d_ac, self.m, None, None, 0, self.roots, self.depths)

    def run_plain(self):
        f = self.f
        f.ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, self.d_ot, self.d_ol, self.k, out=self.plain, arity=f.arity)

    def verified(self):
        """every opening against its anchor's root through the forest's own verify call -> how many pass"""
        import torch
        f, o = self.f, self.out
        ok = torch.zeros(self.k, dtype=torch.uint8, device=f.d.device)
        f.ctx.merkle_forest_ragged_verify_device(f.tag, o[0], o[1], o[2], o[3], self.D, self.d_oa, self.roots, self.m, ok, self.k, arity=f.arity)
        torch.cuda.synchronize()
        return int(ok.sum())


def _consistency_roots(w):
    """the only other route to the roots alone: consistency extraction plus verification of the same (tree, count) pairs -> (run, roots)"""
    import torch
    f, m, D = w.f, w.m, w.D
    ctx, arity, dev = f.ctx, f.arity, f.d.device
    newc = torch.zeros(m, dtype=torch.int64, device=dev)
    lv = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((m, D, arity - 1, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((m, D), dtype=torch.uint8, device=dev)
    dep = torch.zeros(m, dtype=torch.uint8, device=dev)
    ok = torch.zeros(m, dtype=torch.uint8, device=dev)
    old_out = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    new_roots = f.roots[w.d_at.to(torch.int64)].contiguous()
    extract = ctx.merkle4_forest_ragged_consistency_device if arity == 4 else ctx.merkle2_forest_ragged_consistency_device
    verify = ctx.merkle4_forest_consistency_verify_device if arity == 4 else ctx.merkle2_forest_consistency_verify_device

    def run():
        extract(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, w.d_at, w.d_ac, m, newc, lv, sib, pos, dep, None)
        verify(f.tag, w.d_ac, new_roots, newc, new_roots, lv, sib, pos, dep, D, m, ok, None, 0, old_out, None, None)
    return run, old_out


def _one_tree(ctx, arity, n, m, k, rng, reps, rate):
    """one tree of n leaves, m anchors at random counts below n, k openings of random leaves below their anchor's count"""
    import torch
    f = Forest(ctx, arity, [n], n)
    a_count = rng.integers(1, n, m)  # 1 <= c < n: the consistency route needs a grown tree
    o_anchor = rng.integers(0, m, k)
    o_leaf = (rng.random(k) * a_count[o_anchor]).astype(np.int64)
    w = Anchors(f, np.zeros(m, np.int64), a_count, o_anchor, o_leaf)
    other, other_roots = _consistency_roots(w)
    w.run(count=True), w.run_plain(), other()
    torch.cuda.synchronize()
    r = {"arity": arity, "leaves": n, "anchors": m, "openings": k, "bad": w.bad.tolist(), "digests": int(w.hashed),
         "digests_model": int(sum(FA.old_digests(int(c), arity) for c in a_count)) if m <= 1 << 16 else None,
         "roots_equal_consistency": bool(torch.equal(w.roots, other_roots)), "verified": w.verified()}
    t_all, t_plain, t_roots, t_other = _times([w.run, w.run_plain, w.run_roots, other], reps)
    r.update(anchor_ms=med(t_all), plain_ms=med(t_plain), over_plain=med(t_all) / med(t_plain), plain_spread=max(t_plain) / min(t_plain),
             roots_ms=med(t_roots), consistency_ms=med(t_other), roots_over_consistency=med(t_roots) / med(t_other))
    if rate:  # the chains' digests per second against path_ragged on as many openings of the same depth
        o = w.plain
        back = torch.zeros((k, 4), dtype=torch.int64, device=f.d.device)
        path = lambda: ctx.merkle_path_ragged_device(f.tag, o[0], o[1], o[2], o[3], w.D, back, k, arity=arity)  # noqa: E731
        path()
        t_path = med(_times([path], reps)[0])
        levels = int(o[3].to(torch.int64).sum())
        r.update(path_ms=t_path, path_digests=levels, path_digests_per_s=levels / t_path * 1e3, launched_digests=m * w.D,
                 chain_digests_per_s=m * w.D / med(t_roots) * 1e3)
    return r


ONE_TREE = ("%d anchors, %d openings: %.3f ms against plain openings %.3f ms (ratio %.2f; spread of the plain call %.2f)  roots alone %.3f ms "
            "against consistency extract + verify %.3f ms (ratio %.2f, roots identical %s)  digests needed %d%s  %d of %d openings verify against "
            "their anchor's root, bad %s")


def _one_tree_line(r):
    model = "" if r["digests_model"] is None else " (model %d)" % r["digests_model"]
    s = ONE_TREE % (r["anchors"], r["openings"], r["anchor_ms"], r["plain_ms"], r["over_plain"], r["plain_spread"], r["roots_ms"], r["consistency_ms"],
                    r["roots_over_consistency"], r["roots_equal_consistency"], r["digests"], model, r["verified"], r["openings"], r["bad"])
    if "path_ms" in r:
        s += ("  chains: %d digests launched in %.3f ms = %.1f M digests/s against path_ragged %d digests in %.3f ms = %.1f M digests/s"
              % (r["launched_digests"], r["roots_ms"], r["chain_digests_per_s"] / 1e6, r["path_digests"], r["path_ms"], r["path_digests_per_s"] / 1e6))
    return s


def _mixed(ctx, n_trees, rng, reps):
    """C: one anchor per tree 1 .. 16 leaves back, 1 .. 16 openings per anchor; the plain call, and resize(keep) + openings on the copy"""
    import torch
    top = 4 ** 7
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    f = Forest(ctx, 4, sizes, top)
    a_count = np.maximum(sizes - rng.integers(1, 17, n_trees), 1)
    per = rng.integers(1, 17, n_trees)
    o_anchor = np.repeat(np.arange(n_trees), per)
    o_leaf = (rng.random(o_anchor.size) * a_count[o_anchor]).astype(np.int64)
    w = Anchors(f, np.arange(n_trees), a_count, o_anchor, o_leaf)
    dev = f.d.device
    n_leaves = int(sizes.sum())
    # the copy the other route needs: leaves, offsets, levels and roots of the cut forest
    c_leaves = torch.zeros((n_leaves, 4), dtype=torch.int64, device=dev)
    c_off = torch.zeros(n_trees + 1, dtype=torch.int64, device=dev)
    c_lv = torch.zeros((TS.levels_bound(n_leaves, n_trees, top, 4), 4), dtype=torch.int64, device=dev)
    c_roots = torch.zeros((n_trees, 4), dtype=torch.int64, device=dev)
    zero_add = torch.zeros(n_trees + 1, dtype=torch.int64, device=dev)
    copy = tuple(torch.zeros_like(t) for t in w.out)

    def resize_route():
        ctx.merkle4_forest_ragged_resize_device(f.tag, f.d, f.d_off, n_trees, top, f.d_lv, w.d_ac, None, zero_add, n_trees, top, c_leaves, c_off, c_lv,
                                                c_roots, None, None)
        ctx.merkle_forest_ragged_openings_device(c_leaves, c_off, n_trees, top, c_lv, w.d_ot, w.d_ol, w.k, out=copy, arity=4)
    w.run(count=True), w.run_plain(), resize_route()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(w.out, copy)) and bool(torch.equal(w.roots, c_roots))
    extra = sum(t.numel() * t.element_size() for t in (c_leaves, c_off, c_lv, c_roots))
    r = {"trees": n_trees, "leaves": n_leaves, "anchors": w.m, "openings": w.k, "bad": w.bad.tolist(), "digests": int(w.hashed),
         "digests_model": int(sum(FA.old_digests(int(c), 4) for c in a_count)), "launched_digests": w.m * w.D, "identical_to_resize_route": same,
         "resize_route_extra_bytes": extra, "verified": w.verified()}
    t_all, t_plain, t_resize = _times([w.run, w.run_plain, resize_route], reps)
    r.update(anchor_ms=med(t_all), plain_ms=med(t_plain), over_plain=med(t_all) / med(t_plain), plain_spread=max(t_plain) / min(t_plain),
             resize_route_ms=med(t_resize), over_resize_route=med(t_all) / med(t_resize))
    return r


def _lengths(ctx, m, rng, reps):
    """D: mixed against equal chain lengths, roots alone"""
    import torch
    n = 4 ** 12
    f = Forest(ctx, 4, [n], n)
    top = int(TS.depth(n, 4))
    # mixed: a random count cut to a random number of trailing zero digits; equal: odd counts above 4^11 (the longest chain)
    zeros = rng.integers(0, top, m)
    mixed = np.maximum((rng.integers(1, n, m) >> (2 * zeros)) << (2 * zeros), 1)
    equal = rng.integers(4 ** 11 + 1, n, m) | 1
    out = {}
    for name, counts in (("mixed", mixed), ("equal", equal)):
        w = Anchors(f, np.zeros(m, np.int64), counts, [], [])
        w.run(count=True)
        torch.cuda.synchronize()
        out[name] = {"w": w, "digests": int(w.hashed), "digests_model": int(sum(FA.old_digests(int(c), 4) for c in counts))}
    t_mixed, t_equal = _times([out["mixed"]["w"].run_roots, out["equal"]["w"].run_roots], reps)
    return {"anchors": m, "launched_digests": m * top, "mixed_ms": med(t_mixed), "equal_ms": med(t_equal), "mixed_over_equal": med(t_mixed) / med(t_equal),
            "mixed_digests": out["mixed"]["digests"], "equal_digests": out["equal"]["digests"],
            "counts_match_model": all(v["digests"] == v["digests_model"] for v in out.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_anchor.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2^14 openings, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "one_tree": []}
    say("python bench_tools/forest_anchor_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    rng = np.random.default_rng(a.seed)
    k = 1 << 14 if a.quick else 1 << 20
    shapes = ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24))
    for name, (arity, n) in zip("AB", shapes):
        for m in (1, 1 << 10, k):
            r = _one_tree(ctx, arity, n, m, k, rng, a.reps, rate=m == k)
            res["one_tree"].append(r)
            say("%s arity %d, one tree of %d leaves: %s" % (name, arity, n, _one_tree_line(r)))
            torch.cuda.empty_cache()
    r = _mixed(ctx, 2000 if a.quick else a.trees, rng, a.reps)
    res["mixed"] = r
    say("C arity 4, %d trees (log-uniform 1..4^7, %d leaves), one anchor per tree 1..16 leaves back, %d openings: %.3f ms against plain openings %.3f ms "
        "(ratio %.2f; spread of the plain call %.2f) and against resize(keep) + openings %.3f ms (ratio %.2f, bytes identical %s), which needs %.1f MB "
        "more device memory; digests needed %d (model %d) of %d launched; %d of %d openings verify, bad %s"
        % (r["trees"], r["leaves"], r["openings"], r["anchor_ms"], r["plain_ms"], r["over_plain"], r["plain_spread"], r["resize_route_ms"], r["over_resize_route"],
           r["identical_to_resize_route"], r["resize_route_extra_bytes"] / 1e6, r["digests"], r["digests_model"], r["launched_digests"], r["verified"],
           r["openings"], r["bad"]))
    torch.cuda.empty_cache()
    r = _lengths(ctx, 1 << 10 if a.quick else 1 << 16, rng, a.reps)
    res["lengths"] = r
    say("D arity 4, one tree of 4^12 leaves, %d anchors, roots alone: mixed chain lengths %.3f ms (%d digests needed) against equal lengths %.3f ms "
        "(%d needed): ratio %.2f; both launch %d digests; counts match the model: %s"
        % (r["anchors"], r["mixed_ms"], r["mixed_digests"], r["equal_ms"], r["equal_digests"], r["mixed_over_equal"], r["launched_digests"], r["counts_match_model"]))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
