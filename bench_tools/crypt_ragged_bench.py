#!/usr/bin/env python3
"""Messages of different lengths encrypted in one call (p252_encrypt_ragged_device_into) against what a caller could do before it.

  (a) equal lengths   n messages all of --max-len scalars through the ragged call, against p252_encrypt_batch_device at that length
                      in the same run: the price of the schedule and of the indirection
  (b) mixed lengths   n messages, lengths uniform in 1..max-len, against the only other route: per distinct length one gather and one
                      fixed-length call (its launches and the synchronisations of its call-table uploads are counted)
  (c) small batches   n = 1, 64 and 8,192 of mixed lengths

Seeded inputs, device events, warm-up, medians of --reps in one run; the shader clock is noted.  Rate = useful permutations per
second, counted per message from the STREAM call sequence as the kernel runs it.  Prints one line per measurement and a final JSON
line; writes profiles/crypt_ragged.txt unless --no-profile (a "## kernel resources" section already in that file is kept).

  python bench_tools/crypt_ragged_bench.py [--quick] [--messages 1048576] [--max-len 42] [--reps 20] [--warmup 3] [--no-profile]
"""
import argparse
import json
import os
import sys

import numpy as np

from _common import ROOT, clock_mhz, dev, event_ms

PROFILE = os.path.join(ROOT, "profiles", "crypt_ragged.txt")
RESOURCES_MARK = "## kernel resources"


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="2^16 messages, 5 repetitions, no profile file")
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--max-len", type=int, default=42)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0xc29b7)
    ap.add_argument("--no-profile", action="store_true", help="do not write profiles/crypt_ragged.txt")
    args = ap.parse_args()
    if args.quick:
        args.messages, args.reps, args.no_profile = min(args.messages, 1 << 16), min(args.reps, 5), True
    return args


def _count(length):
    """permutations of one STREAM encryption of `length` scalars, counted as the kernel runs them: the sponge permutes when a
    position has reached 4 (absorb 2 + 1, squeeze `length` masks, absorb `length`, squeeze the MAC)"""
    perms, pos_a, pos_s = 0, 0, 0
    for kind, cnt in ((0, 2), (0, 1), (1, length), (0, length), (1, 1)):  # 0 absorb, 1 squeeze
        for _ in range(cnt):
            if (pos_a if kind == 0 else pos_s) == 4:
                perms += 1
                pos_a = 0
                if kind == 1:
                    pos_s = 0
            if kind == 0:
                pos_a += 1
            else:
                pos_s += 1
        if kind == 0:
            pos_s = 4
    return perms


def median(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def case(seed, lens):
    import torch
    from poseidon252_amd import synth
    n = len(lens)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=off[1:])
    total = int(off[-1])
    return {"n": n, "lens": np.asarray(lens), "off": off, "d_off": dev(off), "d_msg": synth.splitmix_scalars(seed, total, "cuda:0"),
            "d_sec": synth.splitmix_scalars(seed + 1, 2 * n, "cuda:0"), "d_non": synth.splitmix_scalars(seed + 2, n, "cuda:0"),
            "d_c": torch.zeros((total + n, 4), dtype=torch.int64, device="cuda:0"),
            "perms": int(sum(_count(int(L)) * int(c) for L, c in zip(*np.unique(lens, return_counts=True))))}


def main():
    args = parse()
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import encryption as E
    ctx = P.Context(0)
    n, ml = args.messages, args.max_len
    res = {"messages": n, "max_len": ml, "reps": args.reps, "clock_mhz_before": clock_mhz(ctx)}
    lines = []

    def report(key, label, ms, perms=None):
        res[key] = {"ms": round(ms, 4)}
        if perms:
            res[key]["perm_per_s"] = perms / (ms * 1e-3)
        line = "%-16s %-78s %10.4f ms%s" % (key, label, ms, "  %.4e useful perm/s" % (perms / (ms * 1e-3)) if perms else "")
        lines.append(line)
        print(line)

    def ragged(c):
        E.encrypt_ragged_device(c["d_msg"], c["d_off"], c["d_sec"], c["d_non"], c["d_c"], c["n"], ml, ctx=ctx)

    # (a) equal lengths
    a = case(args.seed, [ml] * n)
    report("a_ragged", "ragged call, %d messages all of %d scalars" % (n, ml), median(lambda: ragged(a), args.reps, args.warmup), a["perms"])
    d_fixed = torch.zeros((n, ml + 1, 4), dtype=torch.int64, device="cuda:0")
    run_fixed = lambda: E.encrypt_batch_device(a["d_msg"], a["d_sec"], a["d_non"], ml, d_fixed, n, ctx=ctx)  # noqa: E731
    report("a_fixed", "p252_encrypt_batch_device %d x %d" % (n, ml), median(run_fixed, args.reps, args.warmup), a["perms"])
    equal = bool(torch.equal(a["d_c"].view(n, ml + 1, 4), d_fixed))
    fixed_rate = res["a_fixed"]["perm_per_s"]
    del a, d_fixed
    torch.cuda.empty_cache()

    # (b) mixed lengths
    lens = np.random.default_rng(args.seed).integers(1, ml + 1, size=n)
    b = case(args.seed + 10, lens)
    report("b_ragged", "ragged call, %d messages, lengths uniform in 1..%d" % (n, ml), median(lambda: ragged(b), args.reps, args.warmup), b["perms"])
    groups = []
    for L in range(1, ml + 1):
        ids = np.nonzero(lens == L)[0]
        if ids.size:
            d_ids = dev(ids)
            rows = (b["d_off"][:-1][d_ids].view(-1, 1) + torch.arange(L, device="cuda:0").view(1, -1)).reshape(-1)  # (index built beforehand: not timed)
            groups.append((L, ids, d_ids, rows, torch.zeros((ids.size, L + 1, 4), dtype=torch.int64, device="cuda:0")))

    def loop():  # per distinct length: one gather of the messages (secrets and nonces too), one fixed-length call
        for L, ids, d_ids, rows, out in groups:
            E.encrypt_batch_device(b["d_msg"][rows], b["d_sec"].view(-1, 2, 4)[d_ids], b["d_non"][d_ids], L, out, ids.size, ctx=ctx)
    report("b_loop", "%d x (gather + p252_encrypt_batch_device), one per length" % len(groups), median(loop, args.reps, args.warmup), b["perms"])
    got = b["d_c"].cpu().numpy()
    for L, ids, _, _, out in groups[:: max(1, len(groups) // 6)]:
        o = out.cpu().numpy()
        equal = equal and all(np.array_equal(got[int(b["off"][i]) + i:int(b["off"][i + 1]) + i + 1], o[k]) for k, i in list(enumerate(ids))[:: max(1, ids.size // 50)])
    res["b_loop"].update({"fixed_calls": len(groups), "launches": 4 * len(groups), "call_table_uploads_each_with_a_device_synchronise": len(groups)})
    del groups
    torch.cuda.empty_cache()

    # (c) small batches
    for m in (1, 64, 8192):
        c = case(args.seed + m, np.random.default_rng(args.seed + m).integers(1, ml + 1, size=m))
        report("c_%d" % m, "ragged call, %d messages, lengths uniform in 1..%d" % (m, ml), median(lambda: ragged(c), args.reps, args.warmup), c["perms"])

    res["clock_mhz_after"] = clock_mhz(ctx)
    res["outputs_equal"] = equal
    res["ragged_over_fixed_equal_lengths"] = res["a_fixed"]["ms"] / res["a_ragged"]["ms"]
    res["ragged_over_per_length_loop"] = res["b_loop"]["ms"] / res["b_ragged"]["ms"]
    res["mixed_rate_over_fixed_rate"] = res["b_ragged"]["perm_per_s"] / fixed_rate
    res["floor_ragged_over_fixed"] = round(0.90 * res["ragged_over_fixed_equal_lengths"], 3)
    res["floor_ragged_over_loop"] = round(0.85 * res["ragged_over_per_length_loop"], 3)
    tail = ["outputs equal: %s" % equal,
            "ragged over fixed, equal lengths (a_fixed / a_ragged):   %.4f   floor (less 10 %%): %.3f" % (res["ragged_over_fixed_equal_lengths"], res["floor_ragged_over_fixed"]),
            "ragged over the per-length loop (b_loop / b_ragged):    %.4f   floor (less 15 %%): %.3f" % (res["ragged_over_per_length_loop"], res["floor_ragged_over_loop"]),
            "mixed lengths' useful permutation rate over a_fixed's:   %.4f" % res["mixed_rate_over_fixed_rate"],
            "per-length loop: %d fixed-length calls, %d launches (gathers included), %d call-table uploads, each behind a device synchronise"
            % (res["b_loop"]["fixed_calls"], res["b_loop"]["launches"], res["b_loop"]["fixed_calls"]),
            "shader clock of a probe wave before / after: %s / %s MHz" % (res["clock_mhz_before"], res["clock_mhz_after"])]
    for t in tail:
        print(t)
    if not args.no_profile:
        kept = []
        if os.path.exists(PROFILE):
            old = open(PROFILE).read()
            if RESOURCES_MARK in old:
                kept = [old[old.index(RESOURCES_MARK):].rstrip("\n")]
        with open(PROFILE, "w") as f:
            f.write("# bench_tools/crypt_ragged_bench.py --messages %d --max-len %d --reps %d: medians of %d in one run, STREAM variant\n" % (n, ml, args.reps, args.reps))
            f.write("\n".join(lines + tail + [""] + kept) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
