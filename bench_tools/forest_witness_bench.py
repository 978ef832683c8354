#!/usr/bin/env python3
"""The openings of marked leaves kept current by the frontier append (p252_merkle{4,2}_forest_frontier_append_witness_device_into)
against (a) the plain frontier append on the same appends — the difference is the upkeep's cost —, (b) the only route without it: the
stored append (p252_merkle{4,2}_forest_ragged_append_device_into) followed by p252_merkle{4,2}_forest_ragged_openings_device of the same
pairs on the grown forest, and (c) one hipMemcpyDtoDAsync of the bytes the witnesses' pass writes: the ceiling of a gather.

  python bench_tools/forest_witness_bench.py [--reps 20] [--out profiles/forest_witness.txt] [--quick] [--plain-only]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock inside
the bracket); the sides alternate in the one process; the frontier calls work in place, so the state and the witnesses are put back
before every launch, outside the bracket; every witness is compared byte for byte with the openings call of route (b); the shader
clock is probed before and after.
A: one tree of 4^12 leaves (arity 4) and of 2^24 leaves (arity 2) receives 2^16 leaves under k = 2^10, 2^16 and 2^20 carried witnesses
at random positions, and under the 2^16 witnesses of the leaves it receives.
B: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7), 1 to 16 leaves appended to
every tree, 1 to 16 carried witnesses per tree.
The bytes the pass reads and writes are counted from the rule by testsupport/forestwitness.py (pass_bytes), per witness and row: the ids,
the depth byte and the tree's two words; per written row its position byte and the siblings it stores, those it copies read as well.
--plain-only times the plain frontier append alone on the A row of arity 4 and on B: run under P252_LIB_PATH with an earlier build of the
library and without, in turn, it shows what the witnesses' hook costs a caller that has none.
Prints one line per workload, writes them to --out, and prints a JSON summary last."""
import argparse
import ctypes
import json
import os

import numpy as np

import _common as C
from _common import ROOT, Case
from testsupport import treeshape as TS
from testsupport.forestwitness import pass_bytes

_hip = None


def _memcpy_dtod(dst, src, n_bytes):
    """hipMemcpyDtoDAsync on the current stream, from the runtime the process already holds"""
    global _hip
    import torch
    if _hip is None:
        # the copy that is mapped already (torch's): a second copy of the runtime would know nothing of these allocations
        with open("/proc/self/maps") as maps:
            loaded = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
        if len(loaded) != 1:
            raise RuntimeError("expected one HIP runtime in the process, found %r" % loaded)
        _hip = ctypes.CDLL(loaded[0])
        _hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        _hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    rc = _hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), n_bytes, torch.cuda.current_stream().cuda_stream)
    if rc:
        raise RuntimeError("hipMemcpyDtoDAsync: %d" % rc)


class Frontier:
    """the frontier state of a Case's old forest and its in-place appends: plain, and with witnesses"""

    def __init__(self, case):
        from poseidon252_amd import merkle as M
        self.case = case
        self.base, _ = M.ForestFrontier.from_forest(case.ctx, case.d, case.d_off, case.T, case.max_old, case.lv, case.roots_old, max_leaves=case.max_new,
                                                    arity=case.arity)
        self.work = M.ForestFrontier(case.ctx, case.T, case.max_new, case.arity, device=case.d.device)
        ctx = case.ctx
        self.plain = ctx.merkle4_forest_frontier_append_device if case.arity == 4 else ctx.merkle2_forest_frontier_append_device
        self.watched = getattr(ctx, "merkle%d_forest_frontier_append_witness_device" % case.arity)

    def restore(self):
        self.work.counts.copy_(self.base.counts), self.work.frontier.copy_(self.base.frontier), self.work.roots.copy_(self.base.roots)

    def append(self):
        c, w = self.case, self.work
        self.plain(c.tag, w.counts, w.frontier, w.roots, c.T, c.max_new, c.d_add, c.d_aoff, None, None)

    def append_watched(self, wit, n_bad=None):
        c, w = self.case, self.work
        self.watched(c.tag, w.counts, w.frontier, w.roots, c.T, c.max_new, c.d_add, c.d_aoff, wit.tree_ids, wit.leaf_ids, wit.k, wit.leaves,
                     wit.siblings, wit.positions, wit.depths, None, None, n_bad)


def _measure(case, sizes, adds, tid, lid, reps):
    import torch
    from poseidon252_amd import merkle as M
    ctx, arity = case.ctx, case.arity
    front = Frontier(case)
    D = int(TS.depth(case.max_new, arity))
    seed, _ = M.ForestWitnesses.from_openings(ctx, case.d, case.d_off, case.T, case.max_old, case.lv, tid, lid, max_leaves=case.max_new, arity=arity)
    wit = M.ForestWitnesses(ctx, len(tid), case.max_new, arity, seed.tree_ids, seed.leaf_ids)
    arrays = lambda w: (w.leaves, w.siblings, w.positions, w.depths)  # noqa: E731

    def restore():
        front.restore()
        for a, b in zip(arrays(wit), arrays(seed)):
            a.copy_(b)
    # route (b): the stored append, then the openings of the same pairs out of the grown forest
    out = tuple(torch.empty_like(a) for a in arrays(wit))

    def stored():
        case.append()
        ctx.merkle_forest_ragged_openings_device(case.a_leaves, case.a_off, case.T, case.max_new, case.a_lv, wit.tree_ids, wit.leaf_ids, wit.k, out=out,
                                                 arity=arity)
    n_bad = torch.zeros(1, dtype=torch.int32, device=case.d.device)
    restore()
    front.append_watched(wit, n_bad)
    stored()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(arrays(wit), out)) and bool(torch.equal(front.work.roots, case.a_roots)) and int(n_bad) == 0
    read, written = pass_bytes(arity, D, sizes, adds, seed.tree_ids.cpu().numpy(), seed.leaf_ids.cpu().numpy())
    src = torch.empty(max(written, 1), dtype=torch.uint8, device=case.d.device)
    dst = torch.empty_like(src)

    def timer(fn):
        restore()
        return C.event_ms(fn)
    t_wit, t_plain, t_stored, t_copy = C.alternate([lambda: front.append_watched(wit), front.append, stored, lambda: _memcpy_dtod(dst, src, written)],
                                                   reps, timer)
    torch.cuda.synchronize()
    upkeep = t_wit - t_plain
    return {"witness_ms": t_wit, "plain_ms": t_plain, "stored_ms": t_stored, "copy_ms": t_copy, "upkeep_ms": upkeep, "read_bytes": read,
            "written_bytes": written, "tb_per_s": (read + written) / (upkeep * 1e-3) / 1e12 if upkeep > 0 else None,
            "copy_over_upkeep": t_copy / upkeep if upkeep > 0 else None, "identical": same, "k": len(tid), "stride": D}


FORMAT = ("with witnesses %.3f ms  (a) plain frontier append %.3f ms: upkeep %+.3f ms  (b) stored append + openings %.3f ms (%.2f of it)  "
          "(c) copy of the %d bytes written %.3f ms  pass reads %d + writes %d bytes: %s TB/s, the copy's time is %s of the upkeep's  "
          "witnesses identical to the openings call %s")


def _line(r):
    num = lambda v, f: f % v if v is not None else "n/a (upkeep within the noise)"  # noqa: E731
    return FORMAT % (r["witness_ms"], r["plain_ms"], r["upkeep_ms"], r["stored_ms"], r["witness_ms"] / r["stored_ms"], r["written_bytes"], r["copy_ms"],
                     r["read_bytes"], r["written_bytes"], num(r["tb_per_s"], "%.3f"), num(r["copy_over_upkeep"], "%.2f"), r["identical"])


def _mixed(a):
    rng = np.random.default_rng(a.seed)
    top = 4 ** 7
    n_trees = 2000 if a.quick else a.trees
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
    return rng, n_trees, sizes, rng.integers(1, 17, n_trees)


def _plain_only(a, ctx, say):
    """the plain entry point alone, on the one-tree row of arity 4 and on the mixed forest"""
    import torch
    res = {}
    rng, n_trees, sizes, every = _mixed(a)
    for name, sz, adds in (("one_tree", [4 ** 8 if a.quick else 4 ** 12], [1 << 10 if a.quick else 1 << 16]), ("mixed", sizes, every)):
        c = Case(ctx, 4, sz, adds)
        front = Frontier(c)
        front.restore()
        front.append()

        def timer(fn):
            front.restore()
            return C.event_ms(fn)
        res[name] = C.median_ms(front.append, a.reps, timer)
        say("plain frontier append, %s: %.4f ms (library: %s)" % (name, res[name], os.environ.get("P252_LIB_PATH") or "this build"))
        del c, front
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_witness.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2,000 trees): a check of the tool, not a measurement")
    ap.add_argument("--plain-only", action="store_true", help="time the plain frontier append alone (for runs that alternate two builds of the library)")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if a.plain_only:
        print(json.dumps({"reps": a.reps, "plain_ms": _plain_only(a, ctx, say), "clock_mhz": C.clock_mhz(ctx)}))
        return
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "a": []}
    say("python bench_tools/forest_witness_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))

    # ---- A: one tree ----
    rng = np.random.default_rng(a.seed)
    m = 1 << 10 if a.quick else 1 << 16
    for arity, n in ((4, 4 ** 8 if a.quick else 4 ** 12), (2, 2 ** 16 if a.quick else 2 ** 24)):
        c = Case(ctx, arity, [n], [m])
        sets = [("%d carried" % k, rng.integers(0, n, k)) for k in ([1 << 6, 1 << 10, 1 << 12] if a.quick else [1 << 10, 1 << 16, 1 << 20])]
        sets.append(("all %d appended leaves marked" % m, np.arange(n, n + m)))
        for name, lid in sets:
            r = dict(_measure(c, [n], [m], np.zeros(len(lid), dtype=np.int64), lid, a.reps), arity=arity, leaves=n, appended=m, witnesses=name)
            res["a"].append(r)
            say("A arity %d, %d leaves + %d, %s (stride %d): %s" % (arity, n, m, name, r["stride"], _line(r)))
        del c
        torch.cuda.empty_cache()

    # ---- B: the mixed forest ----
    rng, n_trees, sizes, every = _mixed(a)
    per_tree = rng.integers(1, 17, n_trees)
    tid = np.repeat(np.arange(n_trees), per_tree)
    lid = (rng.random(tid.size) * sizes[tid]).astype(np.int64)
    c = Case(ctx, 4, sizes, every)
    r = dict(_measure(c, sizes, every, tid, lid, a.reps), trees=n_trees, leaves=int(sizes.sum()), appended=int(every.sum()))
    res["b"] = r
    say("B: %d trees (log-uniform 1..4^7, %d leaves), %d leaves appended, %d carried witnesses (stride %d): %s"
        % (n_trees, r["leaves"], r["appended"], r["k"], r["stride"], _line(r)))
    rows = res["a"] + [r]
    behind = [x for x in rows if x["witness_ms"] > x["stored_ms"]]
    say("rows: %d; behind route (b) on %d of them; upkeep below 10 %% of the plain call (launch-bound) on %d of them"
        % (len(rows), len(behind), sum(1 for x in rows if x["upkeep_ms"] < 0.1 * x["plain_ms"])))
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
