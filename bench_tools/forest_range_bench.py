#!/usr/bin/env python3
"""Whole runs of leaves of a ragged forest (p252_merkle{4,2}_forest_ragged_range_proofs_device_into: the extraction, no digest;
_forest_range_verify_device_into) against the only other route to the same statement, timed in the same run: the shared proof across
the forest (p252_merkle{4,2}_forest_ragged_multiproof_device_into / _verify_device_into) over the explicit (tree id, leaf id) pairs of
the same positions.

  python bench_tools/forest_range_bench.py [--reps 20] [--out profiles/forest_range.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket); the sides of a comparison alternate in the one process; the shader clock is probed before and after.
Per arity, on one tree of 4^12 leaves (arity 2: 2^24): one run of 2^10, 2^16 and 2^20 leaves from an odd offset, and 2^10 runs of 2^10
leaves.  Then the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7, arity 4) with one
run over the middle half of each tree.
Beside the times: the bytes a range proof's sender ships (ids, first leaves, offsets, lengths, the proof scalars in use) against the
multiproof's (12 bytes a pair, the proof, its offsets); the digests of both verifications; and the extraction against a device copy
(torch's copy_) of the bytes it writes: the leaves and the proof rows.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Forest
from testsupport import forestrange as FR


def _measure(f, tid, first, lens, reps):
    """f: a built Forest; the runs (numpy).  -> the times and counts of one workload"""
    import torch
    ctx, arity, m = f.ctx, f.arity, len(tid)
    dev = f.d.device
    loff = C.offsets(lens)
    k = int(loff[-1])
    stride = FR.range_stride(f.max_leaves, arity)
    d_tid, d_first, d_loff = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(first, np.uint64)), C.dev(loff)
    out = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    proof = torch.zeros((m, max(stride, 1), 4), dtype=torch.int64, device=dev)
    plens = torch.zeros(m, dtype=torch.int32, device=dev)
    counts = torch.zeros(m, dtype=torch.int64, device=dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    ok = torch.zeros(m, dtype=torch.uint8, device=dev)
    hashed = torch.zeros(2, dtype=torch.int64, device=dev)
    extract = ctx.merkle4_forest_ragged_range_proofs_device if arity == 4 else ctx.merkle2_forest_ragged_range_proofs_device
    verify = ctx.merkle4_forest_range_verify_device if arity == 4 else ctx.merkle2_forest_range_verify_device

    def run_extract():
        extract(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_first, d_loff, m, k, proof, plens, counts, out, bad[:1])

    def run_verify():
        verify(f.tag, d_tid, counts, d_first, d_loff, m, f.max_leaves, out, k, proof, stride, plens, f.roots, f.n_trees, ok, None, hashed[:1])
    # the same positions as pairs, ascending in (tree, leaf): the runs sorted by tree (one run a tree here, or all in tree 0 and disjoint)
    order = np.lexsort((np.asarray(first), np.asarray(tid)))
    p_tid = np.repeat(np.asarray(tid)[order], np.asarray(lens)[order]).astype(np.uint32)
    p_lid = np.concatenate([np.arange(first[r], first[r] + lens[r], dtype=np.uint64) for r in order])
    dp_tid, dp_lid = C.dev(p_tid), C.dev(p_lid)
    n_leaves = int(f.off[-1])
    bound = ctx.merkle_forest_ragged_multiproof_bound(n_leaves, f.n_trees, f.max_leaves, k, arity=arity)
    m_out = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    m_proof = torch.zeros((max(bound, 1), 4), dtype=torch.int64, device=dev)
    m_off = torch.zeros(f.n_trees + 1, dtype=torch.int64, device=dev)
    m_ok = torch.zeros(f.n_trees, dtype=torch.uint8, device=dev)

    def run_mp_extract():
        ctx.merkle_forest_ragged_multiproof_device(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, dp_tid, dp_lid, k, m_out, m_proof, m_off, bad[1:], arity=arity)
    run_extract(), run_mp_extract()
    torch.cuda.synchronize()
    m_len = int(m_off[-1])

    def run_mp_verify():
        ctx.merkle_forest_ragged_multiproof_verify_device(f.tag, f.d_off, n_leaves, f.n_trees, f.max_leaves, dp_tid, dp_lid, m_out, k, m_proof, m_len, m_off,
                                                          f.roots, m_ok, None, hashed[1:], arity=arity)
    # a device copy of the bytes the extraction writes
    used = int(plens.to(torch.int64).sum())
    src_leaves, src_proof = out.clone(), torch.zeros((max(used, 1), 4), dtype=torch.int64, device=dev)
    dst_leaves, dst_proof = torch.zeros_like(src_leaves), torch.zeros_like(src_proof)

    def run_copy():
        dst_leaves.copy_(src_leaves)
        dst_proof.copy_(src_proof)
    run_copy(), run_verify(), run_mp_verify()
    torch.cuda.synchronize()
    same_leaves = bool(torch.equal(out, m_out))  # (the pairs are the runs' positions in the runs' order)
    t_ext, t_mpe, t_ver, t_mpv, t_cp = C.alternate([run_extract, run_mp_extract, run_verify, run_mp_verify, run_copy], reps, C.event_ms)
    range_bytes = m * (4 + 8 + 8 + 4 + 8) + 8 + used * 32
    mp_bytes = k * 12 + m_len * 32 + (f.n_trees + 1) * 8
    return {"runs": m, "leaves": k, "bad": int(bad[0]), "mp_bad": int(bad[1]), "extract_ms": t_ext, "mp_extract_ms": t_mpe, "extract_speedup": t_mpe / t_ext,
            "copy_ms": t_cp, "extract_over_copy": t_ext / t_cp, "verify_ms": t_ver, "mp_verify_ms": t_mpv, "verify_speedup": t_mpv / t_ver,
            "ok": int(ok.sum()), "mp_ok": int(m_ok.sum()), "digests": int(hashed[0]), "mp_digests": int(hashed[1]), "proof_scalars": used,
            "mp_proof_scalars": m_len, "range_bytes": range_bytes, "mp_bytes": mp_bytes, "leaves_identical": same_leaves}


FORMAT = ("%d run(s), %d leaves: extraction %.3f ms against the multiproof's %.3f ms (x%.1f) and a device copy of its bytes %.3f ms (%.2f of it)  "
          "verification %.3f ms against the multiproof's %.3f ms (x%.2f; digests %d against %d)  ok %d of %d, multiproof ok on %d trees  "
          "proof %d scalars against %d; ids + proof %d bytes against %d (%.4f)")


def _line(r):
    return FORMAT % (r["runs"], r["leaves"], r["extract_ms"], r["mp_extract_ms"], r["extract_speedup"], r["copy_ms"], r["extract_over_copy"], r["verify_ms"],
                     r["mp_verify_ms"], r["verify_speedup"], r["digests"], r["mp_digests"], r["ok"], r["runs"], r["mp_ok"], r["proof_scalars"],
                     r["mp_proof_scalars"], r["range_bytes"], r["mp_bytes"], r["range_bytes"] / r["mp_bytes"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_range.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, runs of 2^6 .. 2^12 leaves, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "one_tree": []}
    say("python bench_tools/forest_range_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    rng = np.random.default_rng(a.seed)
    shapes = ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24))
    one = [1 << 6, 1 << 9, 1 << 12] if a.quick else [1 << 10, 1 << 16, 1 << 20]
    many = (1 << 4, 1 << 6) if a.quick else (1 << 10, 1 << 10)  # (runs, leaves a run)
    for arity, n in shapes:
        f = Forest(ctx, arity, [n], n)
        for length in one:
            r = dict(_measure(f, [0], [12345 % (n - length)], [length], a.reps), arity=arity, tree=n)
            res["one_tree"].append(r)
            say("arity %d, one tree of %d leaves: %s" % (arity, n, _line(r)))
        # disjoint runs at odd starts, ascending
        slots = np.sort(rng.choice(n // (2 * many[1]), size=many[0], replace=False))
        r = dict(_measure(f, np.zeros(many[0], np.uint32), slots * 2 * many[1] + 3, np.full(many[0], many[1]), a.reps), arity=arity, tree=n)
        res["one_tree"].append(r)
        say("arity %d, one tree of %d leaves: %s" % (arity, n, _line(r)))
        del f
        torch.cuda.empty_cache()
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    f = Forest(ctx, 4, sizes, top)
    lens = np.maximum(sizes // 2, 1)
    r = dict(_measure(f, np.arange(n_trees, dtype=np.uint32), sizes // 4, lens, a.reps), arity=4, trees=n_trees)
    res["mixed"] = r
    say("arity 4, %d trees (log-uniform 1..4^7, %d leaves), the middle half of each: %s" % (n_trees, int(sizes.sum()), _line(r)))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
