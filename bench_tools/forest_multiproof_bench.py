#!/usr/bin/env python3
"""The shared proof across a ragged forest (p252_merkle{4,2}_forest_ragged_multiproof_device_into / _verify_device: k (tree, leaf) pairs, one
tree-major proof, one call each) against the calls that served a forest before it.

  python bench_tools/forest_multiproof_bench.py [--reps 20] [--out profiles/forest_multiproof.txt] [--quick]

(a) --trees mixed trees (leaf counts log-uniform in [1, 4^7], the mix of forest_openings_bench.py), 1 .. 16 pairs per tree: one
    extraction + one verification against the per-tree loop of p252_merkle4_multiproof_device / _verify_device over the tree blocks;
(b) 2^20 random leaves of one 4^12-leaf tree alone in a forest (arity 2: 2^24 leaves) against the single-tree calls on the same positions;
(c) the forest of (a) against p252_merkle4_forest_ragged_openings_device + _forest_ragged_verify_device on the same pairs: proof bytes,
    digests and time, and the same with ONE pair per tree (where the per-leaf openings have nothing to share).
Every shape is warmed up; times are medians of --reps host wall clocks around calls that end in a device synchronise; the two sides of a
ratio alternate in the one process (the per-tree loop of (a), thousands of calls a repetition, runs max(3, reps / 4) of them); every forest proof is verified (d_ok = 1 on the trees with pairs, roots = the build's) and its
offsets and digest count are compared with the model (testsupport/multiproofmodel.py) before it is timed; the shader clock is probed before and after.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT
from testsupport import treeshape as TS
# (the numpy model lived in this module once: all of its names stay importable from here)
from testsupport.multiproofmodel import (forest_multiproof_bound, forest_multiproof_counts, forest_multiproof_extract,  # noqa: F401
                                         forest_multiproof_roots, forest_pairs_by_tree)


# ---------------------------------------------------------------------------------------------
class Forest:
    """a built forest on the device and the buffers of both calls for one set of pairs"""

    def __init__(self, ctx, arity, sizes, tid, lid, seed=5):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.arity, self.sizes = ctx, arity, np.asarray(sizes, dtype=np.int64)
        self.dev = dev = torch.device("cuda:0")
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        self.T, self.n, self.top = len(sizes), int(self.sizes.sum()), int(self.sizes.max())
        self.off = off = TS.offsets(self.sizes, dtype=np.int64)
        self.lo = TS.offsets(TS.levels_len(self.sizes, arity), dtype=np.int64)
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.leaves = torch.randint(0, 1 << 60, (self.n, 4), dtype=torch.int64, generator=g).to(dev)
        self.offsets = torch.from_numpy(off).to(dev)
        self.levels = torch.zeros((max(TS.levels_bound(self.n, self.T, self.top, arity), 1), 4), dtype=torch.int64, device=dev)
        self.roots = torch.zeros((self.T, 4), dtype=torch.int64, device=dev)
        ctx.merkle_forest_ragged_device(self.tag, self.leaves, self.offsets, self.T, self.top, self.roots, d_levels=self.levels, arity=arity)
        self.set_pairs(tid, lid)

    def set_pairs(self, tid, lid):
        import torch
        dev, ctx = self.dev, self.ctx
        self.tid_h, self.lid_h = np.asarray(tid, dtype=np.int64), np.asarray(lid, dtype=np.int64)
        self.k = k = self.tid_h.size
        self.tid = torch.from_numpy(self.tid_h.astype(np.int32)).to(dev)
        self.lid = torch.from_numpy(self.lid_h).to(dev)
        bound_fn = ctx.merkle4_forest_ragged_multiproof_bound if self.arity == 4 else ctx.merkle2_forest_ragged_multiproof_bound
        self.bound = bound_fn(self.n, self.T, self.top, k)
        self.out = torch.empty((k, 4), dtype=torch.int64, device=dev)
        self.proof = torch.empty((max(self.bound, 1), 4), dtype=torch.int64, device=dev)
        self.po = torch.zeros(self.T + 1, dtype=torch.int64, device=dev)
        self.ok = torch.zeros(self.T, dtype=torch.uint8, device=dev)
        self.roots_out = torch.zeros((self.T, 4), dtype=torch.int64, device=dev)
        self.hashed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.length = 0

    def extract(self):
        c = self.ctx
        f = c.merkle4_forest_ragged_multiproof_device if self.arity == 4 else c.merkle2_forest_ragged_multiproof_device
        f(self.leaves, self.offsets, self.T, self.top, self.levels, self.tid, self.lid, self.k, self.out, self.proof, self.po)

    def verify(self):
        c = self.ctx
        f = c.merkle4_forest_ragged_multiproof_verify_device if self.arity == 4 else c.merkle2_forest_ragged_multiproof_verify_device
        f(self.tag, self.offsets, self.n, self.T, self.top, self.tid, self.lid, self.out, self.k, self.proof if self.length else None, self.length,
          self.po, self.roots, self.ok, d_roots_out=self.roots_out, d_n_hashed=self.hashed)

    def check(self):
        """both calls once; True iff offsets and digest count are the model's and every tree with a pair verifies to the build's root"""
        import torch
        self.extract()
        self.length = int(self.po[-1])
        self.verify()
        torch.cuda.synchronize()
        want_po, want_hashed = forest_multiproof_counts(self.sizes, self.tid_h, self.lid_h, self.arity)
        has = np.zeros(self.T, dtype=bool)
        has[self.tid_h] = True
        hm = torch.from_numpy(has).to(self.dev)
        return (np.array_equal(self.po.cpu().numpy().astype(np.uint64), want_po) and int(self.hashed) == want_hashed and
                np.array_equal(self.ok.cpu().numpy().astype(bool), has) and bool(torch.equal(self.roots_out[hm], self.roots[hm])))

    def per_tree_loop(self):
        """(extract, verify) that serve the same pairs with the single-tree calls, one tree block at a time"""
        import torch
        ctx, a, dev = self.ctx, self.arity, self.dev
        per = forest_pairs_by_tree(self.T, self.tid_h, self.lid_h)
        jobs, at = [], 0
        for t in sorted(per):
            n, kt = int(self.sizes[t]), per[t].size
            idx = torch.from_numpy(per[t].astype(np.int32)).to(dev)
            lv = self.levels[self.lo[t]:self.lo[t + 1]] if n > 1 else None
            proof = torch.empty((max(ctx.merkle_multiproof_bound(n, kt, a), 1), 4), dtype=torch.int64, device=dev)
            jobs.append((t, n, kt, idx, self.leaves[self.off[t]:self.off[t + 1]], lv, torch.empty((kt, 4), dtype=torch.int64, device=dev), proof,
                         int(self.po[t + 1] - self.po[t])))
            at += kt
        plen = torch.zeros(1, dtype=torch.int64, device=dev)
        ok1 = torch.zeros(1, dtype=torch.uint8, device=dev)

        def extract():
            for t, n, kt, idx, lf, lv, out, proof, length in jobs:
                ctx.merkle_multiproof_device(lf, n, lv, idx, kt, out, proof, plen, arity=a)

        def verify():
            for t, n, kt, idx, lf, lv, out, proof, length in jobs:
                ctx.merkle_multiproof_verify_device(self.tag, n, idx, out, kt, proof if length else None, length, self.roots[t], ok1, arity=a)
        return extract, verify


def mixed_forest(n_trees, lo_pairs, hi_pairs, seed=7, top=4 ** 7):
    """the size mix of forest_openings_bench.py (log-uniform in [1, top]) and lo .. hi random pairs per tree, ascending"""
    rng = np.random.default_rng(seed)
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    tid, lid = [], []
    for t, n in enumerate(sizes):
        kt = min(int(rng.integers(lo_pairs, hi_pairs + 1)), int(n))
        pos = np.sort(rng.choice(int(n), kt, replace=False))
        tid.append(np.full(kt, t, dtype=np.int64))
        lid.append(pos.astype(np.int64))
    return sizes, np.concatenate(tid), np.concatenate(lid)


def _openings_side(f):
    """the per-leaf forest openings + verify on f's pairs: (extract, verify, siblings bytes, digests)"""
    import torch
    ctx, dev, k = f.ctx, f.dev, f.k
    lv, sib, pos, dep, D = ctx.merkle_forest_ragged_openings_device(f.leaves, f.offsets, f.T, f.top, f.levels, f.tid, f.lid, k, arity=f.arity)
    bufs = (lv, sib, pos, dep)
    oks = torch.zeros(k, dtype=torch.uint8, device=dev)
    extract = lambda: ctx.merkle_forest_ragged_openings_device(f.leaves, f.offsets, f.T, f.top, f.levels, f.tid, f.lid, k, out=bufs, arity=f.arity)  # noqa: E731
    verify = lambda: ctx.merkle_forest_ragged_verify_device(f.tag, lv, sib, pos, dep, D, f.tid, f.roots, f.T, oks, k, arity=f.arity)  # noqa: E731
    verify()
    torch.cuda.synchronize()
    depths = TS.depth(f.sizes, f.arity)[f.tid_h]
    return extract, verify, int(depths.sum()) * (f.arity - 1) * 32, int(depths.sum()), int(oks.sum()) == k


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_multiproof.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (500 trees; 4^8 and 2^16 leaves): a check of the tool, not a measurement")
    a = ap.parse_args()
    import poseidon252_amd as P
    import torch
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx)}
    say("python bench_tools/forest_multiproof_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    n_trees = 500 if a.quick else a.trees
    loop_reps = max(3, a.reps // 4)  # (the loop is thousands of launch-bound calls a repetition)

    # ---- (a) and (c): the mixed forest ----
    sizes, tid, lid = mixed_forest(n_trees, 1, 16)
    f = Forest(ctx, 4, sizes, tid, lid)
    good = f.check()
    loop_extract, loop_verify = f.per_tree_loop()
    loop_extract(), loop_verify()
    t_loop_e, t_e = C.alternate([loop_extract, f.extract], loop_reps, C.once_ms)
    t_loop_v, t_v = C.alternate([loop_verify, f.verify], loop_reps, C.once_ms)
    res["a"] = {"trees": n_trees, "leaves": f.n, "pairs": f.k, "loop_extract_ms": t_loop_e, "forest_extract_ms": t_e, "extract_ratio": t_loop_e / t_e,
                "loop_verify_ms": t_loop_v, "forest_verify_ms": t_v, "verify_ratio": t_loop_v / t_v, "agrees_with_model": good}
    say("(a) %d mixed trees, %d leaves, %d pairs (1 .. 16 a tree): extract per-tree loop %.2f ms  one call %.3f ms  ratio %.1f  |  verify "
        "per-tree loop %.2f ms  one call %.3f ms  ratio %.1f  agrees with the model %s"
        % (n_trees, f.n, f.k, t_loop_e, t_e, t_loop_e / t_e, t_loop_v, t_v, t_loop_v / t_v, good))
    for label, (lo_p, hi_p) in (("1 .. 16 pairs a tree", (1, 16)), ("1 pair a tree", (1, 1)), ("2 pairs a tree", (2, 2)), ("4 pairs a tree", (4, 4))):
        _, tid_c, lid_c = mixed_forest(n_trees, lo_p, hi_p)
        f.set_pairs(tid_c, lid_c)
        good = f.check()
        o_e, o_v, o_bytes, o_digests, o_ok = _openings_side(f)
        t_oe, t_me = C.alternate([o_e, f.extract], a.reps, C.once_ms)
        t_ov, t_mv = C.alternate([o_v, f.verify], a.reps, C.once_ms)
        row = {"pairs_per_tree": label, "pairs": f.k, "openings_ms": t_oe, "multiproof_ms": t_me, "extract_ratio": t_oe / t_me, "verify_ms": t_ov,
               "multiproof_verify_ms": t_mv, "verify_ratio": t_ov / t_mv, "siblings_bytes": o_bytes, "proof_bytes": f.length * 32,
               "digests_per_leaf": o_digests, "digests_once": int(f.hashed), "agrees_with_model": good and o_ok}
        res.setdefault("c", []).append(row)
        say("(c) %d mixed trees, %s (%d pairs): extract openings %.3f ms (%d B)  multiproof %.3f ms (%d B)  ratio %.2f (bytes %.2f)  |  verify "
            "per leaf %.3f ms (%d digests)  multiproof %.3f ms (%d digests)  ratio %.2f (digests %.2f)  agrees with the model %s"
            % (n_trees, label, f.k, t_oe, o_bytes, t_me, f.length * 32, t_oe / t_me, o_bytes / max(f.length * 32, 1), t_ov, o_digests, t_mv,
               int(f.hashed), t_ov / t_mv, o_digests / max(int(f.hashed), 1), good and o_ok))
    del f
    torch.cuda.empty_cache()

    # ---- (b): one large tree alone in a forest ----
    res["b"] = []
    for arity, n, k in ((4, 4 ** 8 if a.quick else 4 ** 12, 1 << (12 if a.quick else 20)), (2, 2 ** 16 if a.quick else 2 ** 24, 1 << (12 if a.quick else 20))):
        pos = np.sort(np.random.default_rng(1).choice(n, k, replace=False)).astype(np.int64)
        f = Forest(ctx, arity, [n], np.zeros(k, dtype=np.int64), pos)
        good = f.check()
        idx = torch.from_numpy(pos.astype(np.uint32).view(np.int32)).to(f.dev)
        out1 = torch.empty((k, 4), dtype=torch.int64, device=f.dev)
        proof1 = torch.empty((ctx.merkle_multiproof_bound(n, k, arity), 4), dtype=torch.int64, device=f.dev)
        plen, ok1 = torch.zeros(1, dtype=torch.int64, device=f.dev), torch.zeros(1, dtype=torch.uint8, device=f.dev)
        single_e = lambda: ctx.merkle_multiproof_device(f.leaves, n, f.levels, idx, k, out1, proof1, plen, arity=arity)  # noqa: E731
        single_e()
        length = int(plen)
        single_v = lambda: ctx.merkle_multiproof_verify_device(f.tag, n, idx, out1, k, proof1, length, f.roots[0], ok1, arity=arity)  # noqa: E731
        single_v()
        torch.cuda.synchronize()
        good = good and length == f.length and int(ok1) == 1 and bool(torch.equal(proof1[:length], f.proof[:length]))
        t_se, t_fe = C.alternate([single_e, f.extract], a.reps, C.once_ms)
        t_sv, t_fv = C.alternate([single_v, f.verify], a.reps, C.once_ms)
        res["b"].append({"arity": arity, "leaves": n, "k": k, "single_extract_ms": t_se, "forest_extract_ms": t_fe, "extract_ratio": t_se / t_fe,
                         "single_verify_ms": t_sv, "forest_verify_ms": t_fv, "verify_ratio": t_sv / t_fv, "agrees": good})
        say("(b) arity %d, one tree of %d leaves alone in a forest, k = 2^%d: extract single-tree %.3f ms  forest %.3f ms  ratio %.2f  |  verify "
            "single-tree %.3f ms  forest %.3f ms  ratio %.2f  same bytes and verdict %s"
            % (arity, n, int(np.log2(k)), t_se, t_fe, t_se / t_fe, t_sv, t_fv, t_sv / t_fv, good))
        del f, out1, proof1
        torch.cuda.empty_cache()
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
