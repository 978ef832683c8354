#!/usr/bin/env python3
"""Messages of different lengths: one ragged call (p252_hash_ragged_device) against what a caller could do before it.

  (a) ragged    the ragged call, sorted schedule (default)
  (b) unsorted  the same call under P252_RAGGED_SORT=0 — run in a fresh child process (the switch is read once per process)
  (c) uniform   p252_hash_batch_device on n x max_len -> out_len: the uniform reference of the committed sponge rate
  (d) grouped   one p252_hash_batch_device per distinct length on buffers gathered beforehand (kernel time only)

Seeded inputs (lengths uniform in 1..max_len, scalars from synth.splitmix_scalars), device events, warm-up, median of --reps.
Rate = useful permutations per second, useful = sum over messages of ceil(L/4) + ceil(out_len/4) - 1.  The outputs of (a), (b)
and (d) are compared byte for byte.  Prints one line per measurement and a final JSON line.

  python bench_tools/ragged_bench.py [--messages 1048576] [--max-len 42] [--out-len 1] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--max-len", type=int, default=42)
    ap.add_argument("--out-len", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x7a99ed)
    ap.add_argument("--skip", default="", help="comma-separated subset of a,b,c,d not to run")
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)  # (b): run (a) only, save the outputs here
    return ap.parse_args()


def inputs(args, dev):
    import numpy as np
    import torch
    from poseidon252_amd import synth
    rng = np.random.default_rng(args.seed)
    lens = rng.integers(1, args.max_len + 1, size=args.messages).astype(np.uint64)
    off = np.zeros(args.messages + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = synth.splitmix_scalars(args.seed, int(off[-1]), dev)
    return lens, off, flat, torch.from_numpy(off.view(np.int64)).to(dev)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    args = parse()
    import numpy as np
    import torch
    import poseidon252_amd as P
    dev = torch.device("cuda", 0)
    ctx = P.Context(0)
    skip = set(filter(None, args.skip.split(",")))
    lens, off, d_flat, d_off = inputs(args, dev)
    n, ol = args.messages, args.out_len
    blocks = (lens.astype(np.int64) + 3) // 4
    useful = int(blocks.sum()) + n * ((ol + 3) // 4 - 1)
    rb = P.RaggedHashBatch(P.Domain.Other, output_len=ol, ctx=ctx)
    out_a = torch.empty((n, ol, 4), dtype=torch.int64, device=dev)
    run_a = lambda: rb.digest((d_flat, d_off), max_len=args.max_len, out=out_a)  # noqa: E731
    ms_a = timed(run_a, args.reps, args.warmup)
    if args.child_out:
        np.save(args.child_out, out_a.cpu().numpy())
        print(json.dumps({"ms": ms_a}))
        return
    res = {"messages": n, "max_len": args.max_len, "out_len": ol, "useful_perms": useful, "reps": args.reps,
           "sort": os.environ.get("P252_RAGGED_SORT", "1") != "0"}

    def report(key, label, ms, perms):
        res[key] = {"ms": round(ms, 4), "perm_per_s": perms / (ms * 1e-3)}
        print("%-10s %-62s %9.3f ms  %.4e useful perm/s" % (key, label, ms, perms / (ms * 1e-3)))

    report("a", "ragged call, sorted (lengths 1..%d)" % args.max_len, ms_a, useful)
    got_a = out_a.cpu().numpy()
    equal = {}
    if "b" not in skip:  # a fresh process: P252_RAGGED_SORT is read once per process
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ragged_bench_b_%d.npy" % os.getpid())
        env = dict(os.environ, P252_RAGGED_SORT="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--messages", str(n), "--max-len", str(args.max_len), "--out-len", str(ol),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--seed", str(args.seed), "--child-out", path]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
        if r.returncode != 0:
            raise SystemExit("unsorted child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        report("b", "ragged call, P252_RAGGED_SORT=0 (child process)", json.loads(r.stdout.strip().splitlines()[-1])["ms"], useful)
        equal["a_b"] = bool(np.array_equal(np.load(path), got_a))
        os.remove(path)
    if "c" not in skip:
        hb = P.HashBatch(P.Domain.Other, args.max_len, output_len=ol, ctx=ctx)
        d_u = d_flat[: n * args.max_len] if d_flat.shape[0] >= n * args.max_len else synth_uniform(args, n, dev)
        out_c = torch.empty((n, ol, 4), dtype=torch.int64, device=dev)
        ms_c = timed(lambda: hb.digest(d_u, out=out_c), args.reps, args.warmup)
        report("c", "uniform: p252_hash_batch_device %d x %d -> %d" % (n, args.max_len, ol), ms_c,
               n * (((args.max_len + 3) // 4) + (ol + 3) // 4 - 1))
        del d_u
    if "d" not in skip:
        groups = []
        idx_all = np.arange(n)
        for L in range(1, args.max_len + 1):
            idx = idx_all[lens == L]
            if not idx.size:
                continue
            d_idx = torch.from_numpy(idx).to(dev)
            rows = (d_off[:-1][d_idx].view(-1, 1) + torch.arange(L, device=dev).view(1, -1)).reshape(-1)
            gathered = d_flat[rows].contiguous()  # pre-gathered: not timed
            groups.append((L, d_idx, gathered, torch.empty((idx.size, ol, 4), dtype=torch.int64, device=dev),
                           P.HashBatch(P.Domain.Other, L, output_len=ol, ctx=ctx)))
        torch.cuda.synchronize()

        def run_d():
            for L, _, g, o, hb in groups:
                hb.digest(g, out=o)
        ms_d = timed(run_d, args.reps, args.warmup)
        report("d", "grouped: %d p252_hash_batch_device calls, one per length" % len(groups), ms_d, useful)
        out_d = torch.empty((n, ol, 4), dtype=torch.int64, device=dev)
        for L, d_idx, _, o, _ in groups:
            out_d[d_idx] = o
        equal["a_d"] = bool(np.array_equal(out_d.cpu().numpy(), got_a))
        del groups
    res["outputs_equal"] = equal
    if "b" in res:
        res["sorted_over_unsorted"] = res["b"]["ms"] / res["a"]["ms"]
    if "c" in res:
        res["ragged_rate_over_uniform"] = res["a"]["perm_per_s"] / res["c"]["perm_per_s"]
    if "d" in res:
        res["ragged_over_grouped"] = res["d"]["ms"] / res["a"]["ms"]
    print("outputs equal: %s" % equal)
    print(json.dumps(res))


def synth_uniform(args, n, dev):
    from poseidon252_amd import synth
    return synth.splitmix_scalars(args.seed + 1, n * args.max_len, dev)


if __name__ == "__main__":
    main()
