#!/usr/bin/env python3
"""Many leaves of ONE tree behind one shared proof (p252_merkle{4,2}_multiproof_device / _verify_device, every ancestor hashed once)
against the per-leaf calls (p252_merkle{4,2}_openings_device, p252_merkle{4,2}_verify_batch_device) on the same leaves.

  python bench_tools/multiproof_bench.py [--reps 20] [--out profiles/multiproof.txt] [--quick]

One arity-4 tree of 4^12 leaves and one arity-2 tree of 2^24 leaves; k = 2^10, 2^14, 2^17, 2^20 random distinct positions (seed 1),
sorted.  Every shape is warmed up; times are medians of --reps host wall clocks around calls that end in a device synchronise; the
two sides of a ratio alternate in the one process; every multiproof is verified (ok = 1, root = the tree's) and its length and digest
count are compared with the numpy model (testsupport/multiproofmodel.py) before it is timed; the shader clock is probed before and after.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT
from testsupport.device import tree_device
# (the numpy model lived in this module once: all of its names stay importable from here)
from testsupport.multiproofmodel import multiproof_bound, multiproof_counts, multiproof_extract, multiproof_model, multiproof_root  # noqa: F401


def _tree(ctx, arity, n, say, reps, ks):
    import torch
    from poseidon252_amd import merkle as M
    dev = torch.device("cuda:0")
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    d = torch.randint(0, 1 << 60, (n, 4), dtype=torch.int64, device=dev)
    root = torch.empty(4, dtype=torch.int64, device=dev)
    lv = torch.empty((M.levels_len(n, arity), 4), dtype=torch.int64, device=dev)
    tree_device(ctx, arity, tag, d, n, root, lv)
    rows = []
    for k in ks:
        pos = np.sort(np.random.default_rng(1).choice(n, k, replace=False)).astype(np.uint32)
        d_idx = torch.from_numpy(pos.view(np.int32)).to(dev)
        want_len, want_hashed = multiproof_counts(n, pos, arity)
        bound = ctx.merkle_multiproof_bound(n, k, arity)
        out = torch.empty((k, 4), dtype=torch.int64, device=dev)
        proof = torch.empty((bound, 4), dtype=torch.int64, device=dev)
        plen, hashed = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        ok, root_out = torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        extract = lambda: ctx.merkle_multiproof_device(d, n, lv, d_idx, k, out, proof, plen, arity=arity)  # noqa: E731
        extract()
        length = int(plen)
        verify = lambda: ctx.merkle_multiproof_verify_device(tag, n, d_idx, out, k, proof, length, root, ok, d_root_out=root_out,  # noqa: E731
                                                             d_n_hashed=hashed, arity=arity)
        verify()
        torch.cuda.synchronize()
        good = length == want_len and int(hashed) == want_hashed and int(ok) == 1 and bool(torch.equal(root_out, root))
        # the per-leaf calls on the same leaves
        o_l, o_s, o_p, depth = ctx.merkle4_openings_device(d, n, lv, d_idx, k, arity=arity)
        bufs = (o_l, o_s, o_p, torch.zeros(1, dtype=torch.int32, device=dev))
        openings = lambda: ctx.merkle4_openings_device(d, n, lv, d_idx, k, out=bufs, arity=arity)  # noqa: E731
        oks = torch.zeros(k, dtype=torch.uint8, device=dev)
        batch = lambda: ctx.merkle_verify_batch_device(tag, o_l, o_s, o_p, depth, root, oks, k, arity=arity)  # noqa: E731
        batch()
        torch.cuda.synchronize()
        good = good and int(oks.sum()) == k
        t_open, t_extract = C.alternate([openings, extract], reps, C.once_ms)
        t_batch, t_verify = C.alternate([batch, verify], reps, C.once_ms)
        per_leaf_scalars, per_leaf_digests = k * depth * (arity - 1), k * depth
        rows.append({"arity": arity, "leaves": n, "k": k, "openings_ms": t_open, "multiproof_ms": t_extract, "extract_ratio": t_open / t_extract,
                     "verify_batch_ms": t_batch, "multiproof_verify_ms": t_verify, "verify_ratio": t_batch / t_verify,
                     "siblings_bytes": per_leaf_scalars * 32, "proof_bytes": length * 32, "bytes_ratio": per_leaf_scalars / max(length, 1),
                     "digests_per_leaf": per_leaf_digests, "digests_once": int(hashed), "digest_ratio": per_leaf_digests / int(hashed),
                     "bound": bound, "agrees_with_model": good})
        say("arity %d, %d leaves, k = 2^%d: extract openings %.3f ms (%d B)  multiproof %.3f ms (%d B; bound %d B)  ratio %.2f (bytes %.2f)  |  "
            "verify_batch %.3f ms (%d digests)  multiproof_verify %.3f ms (%d digests)  ratio %.2f (digests %.2f)  agrees with the model %s"
            % (arity, n, int(np.log2(k)), t_open, per_leaf_scalars * 32, t_extract, length * 32, bound * 32, t_open / t_extract,
               per_leaf_scalars / max(length, 1), t_batch, per_leaf_digests, t_verify, int(hashed), t_batch / t_verify,
               per_leaf_digests / int(hashed), good))
        del out, proof, o_l, o_s, o_p, bufs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiproof.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 and 2^16 leaves): a check of the tool, not a measurement")
    ap.add_argument("--only", type=int, default=0, help="one k of one arity-4 tree only (for a profiler run)")
    a = ap.parse_args()
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx)}
    say("python bench_tools/multiproof_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    ks = [1 << 6, 1 << 10, 1 << 14] if a.quick else [1 << 10, 1 << 14, 1 << 17, 1 << 20]
    if a.only:
        res["rows"] = _tree(ctx, 4, 4 ** 12, say, a.reps, [a.only])
    else:
        res["rows"] = _tree(ctx, 4, 4 ** 8 if a.quick else 4 ** 12, say, a.reps, ks)
        res["rows"] += _tree(ctx, 2, 2 ** 16 if a.quick else 2 ** 24, say, a.reps, ks)
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
