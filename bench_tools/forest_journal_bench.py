#!/usr/bin/env python3
"""Leaf updates of a ragged forest that keep a journal (p252_merkle{4,2}_forest_ragged_update_journaled_device_into) and the swap that undoes
them (p252_merkle{4,2}_forest_ragged_journal_swap_device_into) against what a caller has without them.

  python bench_tools/forest_journal_bench.py [--reps 20] [--out profiles/forest_journal.txt] [--quick]

Per case, in one process, every callable warmed up, medians of --reps host wall clocks around calls that end in a device synchronise,
the two sides of a ratio alternating:
  (a) the journaled update against the plain update (p252_merkle{4,2}_forest_ragged_update_device) on the same inputs: what the journal
      costs on the way in;
  (b) one swap against a plain update with the saved old leaves, which is how a caller leaves an update without a journal.  Before the
      timing the round trip is checked byte for byte: update, swap (= the forest before), swap (= the forest after).  While timing,
      the swap and the re-update alternate on one forest, so the swap then exchanges whatever the forest holds: the same entries, the
      same bytes moved;
  and the swap's bytes per second — 32 bytes read and 32 written on either side of each entry, ids apart — against a device-to-device
  copy that moves the same bytes (64 bytes per entry read, 64 written), both with their launch overheads.
Cases: ONE arity-4 tree of 4^12 leaves with k = 1, 2^10, 2^16, 2^20 distinct random leaves (seed 1); one arity-2 tree of 2^24 leaves
with the same k; --trees mixed trees (leaf counts log-uniform in [1, 4^7], seed 7) with 1 - 16 updates each (at most the tree's
leaves).  Prints one line per case, writes them to --out, and prints a JSON summary last."""
import argparse
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Forest
from testsupport import treeshape as TS
from testsupport.forestupdate import dirty_nodes


def _case(ctx, name, f, tid, lid, reps, say):
    """one forest, one update list -> the row of results"""
    import torch
    a, k = f.arity, len(tid)
    d_tid, d_lid = C.dev(np.asarray(tid, np.uint32)), C.dev(np.asarray(lid, np.uint64))
    slot = C.dev(f.off[np.asarray(tid)].astype(np.int64) + np.asarray(lid, np.int64))
    d_old = f.d[slot].clone()  # what a caller without a journal must have saved
    d_new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(3))
    n_leaves = f.d.shape[0]
    cap = getattr(ctx, "merkle%d_forest_ragged_journal_bound" % a)(n_leaves, f.n_trees, f.max_leaves, k)
    ids = torch.zeros((cap, 4), dtype=torch.int32, device="cuda:0")
    values = torch.zeros((cap, 4), dtype=torch.int64, device="cuda:0")
    jlen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    upd_j, swap_j = getattr(ctx, "merkle%d_forest_ragged_update_journaled_device" % a), getattr(ctx, "merkle%d_forest_ragged_journal_swap_device" % a)

    def plain(leaves=d_new):
        ctx.merkle_forest_ragged_update_device(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_lid, leaves, k, d_roots=f.roots, arity=a)

    def journaled(count=None):
        upd_j(f.tag, f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_tid, d_lid, d_new, k, ids, values, cap, jlen, d_roots=f.roots, d_n_hashed=count)

    def swap():
        swap_j(f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, ids, values, cap, jlen, d_roots=f.roots)

    def reupdate():
        plain(d_old)
    # the round trip, byte for byte
    before = (f.d.clone(), f.d_lv.clone(), f.roots.clone())
    journaled(hashed)
    after = (f.d.clone(), f.d_lv.clone(), f.roots.clone())
    swap()
    undone = all(bool(torch.equal(x, y)) for x, y in zip((f.d, f.d_lv, f.roots), before))
    swap()
    redone = all(bool(torch.equal(x, y)) for x, y in zip((f.d, f.d_lv, f.roots), after))
    plain()
    same = all(bool(torch.equal(x, y)) for x, y in zip((f.d, f.d_lv, f.roots), after))  # the plain update writes the same forest
    n_entries, n_hashed = int(jlen), int(hashed)
    # (a)
    plain(), journaled()
    t_plain, t_journaled = C.alternate([plain, journaled], reps, C.once_ms)
    # (b)
    journaled(), swap(), reupdate()
    t_swap, t_re = C.alternate([swap, reupdate], reps, C.once_ms)
    # the swap's bytes against a copy of the same bytes
    src = torch.empty(max(n_entries, 1) * 64, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)  # noqa: E731
    copy()
    t_swap2, t_copy = C.alternate([swap, copy], reps, C.once_ms)
    moved = n_entries * 128
    row = {"case": name, "arity": a, "k": k, "journal_entries": n_entries, "journal_bound": cap, "digests": n_hashed,
           "digests_numpy": dirty_nodes(f.sizes, tid, lid, a), "plain_update_ms": t_plain, "journaled_update_ms": t_journaled,
           "journaled_over_plain": t_journaled / t_plain, "swap_ms": t_swap, "reupdate_ms": t_re, "reupdate_over_swap": t_re / t_swap,
           "swap_gb_s": moved / t_swap2 / 1e6, "copy_gb_s": moved / t_copy / 1e6, "swap_of_copy": t_copy / t_swap2,
           "undo_identical": undone, "redo_identical": redone, "plain_identical": same}
    say("%s, k = %d: plain update %.3f ms  journaled %.3f ms (x%.3f; %d entries of at most %d, %d digests)  |  swap %.3f ms  re-update with the "
        "old leaves %.3f ms  re-update/swap %.2f  |  swap %.1f GB/s, a copy of the same bytes %.1f GB/s (%.2f of it)  |  undo identical %s, "
        "redo identical %s, plain update identical %s"
        % (name, k, t_plain, t_journaled, t_journaled / t_plain, n_entries, cap, n_hashed, t_swap, t_re, t_re / t_swap, row["swap_gb_s"],
           row["copy_gb_s"], row["swap_of_copy"], undone, redone, same))
    f.build()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_journal.txt"), help="where the case lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (a 4^8-leaf tree, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "rows": []}
    say("python bench_tools/forest_journal_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    ks = [1, 1 << 6, 1 << 12] if a.quick else [1, 1 << 10, 1 << 16, 1 << 20]
    for arity, n in ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24)):
        f = Forest(ctx, arity, [n], n)
        for k in ks:
            lid = np.random.default_rng(1).choice(n, k, replace=False)
            res["rows"].append(_case(ctx, "arity %d, one tree of %d^%d leaves" % (arity, arity, TS.depth(n, arity)), f, np.zeros(k, np.int64), lid, a.reps, say))
        del f
        torch.cuda.empty_cache()
    rng = np.random.default_rng(a.seed)
    top, n_trees = 4 ** 7, 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    per = np.minimum(rng.integers(1, 17, n_trees), sizes)
    tid = np.repeat(np.arange(n_trees), per)
    lid = np.concatenate([rng.choice(int(n), int(m), replace=False) for n, m in zip(sizes, per)])
    f = Forest(ctx, 4, sizes, top)
    res["rows"].append(_case(ctx, "arity 4, %d mixed trees (log-uniform 1..4^7, %d leaves), 1-16 updates each" % (n_trees, int(sizes.sum())), f, tid, lid,
                             a.reps, say))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
