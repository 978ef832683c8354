#!/usr/bin/env python3
"""Trees of built forests gathered into a new compact forest (p252_merkle{4,2}_forest_ragged_select_device_into: leaves, level blocks
and roots relocated, nothing hashed) against a fresh p252_merkle{4,2}_forest_ragged_device build of the same new forest and against a
hipMemcpyDtoDAsync of the same bytes, timed in the same run.

  python bench_tools/forest_select_bench.py [--reps 20] [--cases mixed,one4,one2] [--out profiles/forest_select.txt] [--quick]

Every shape is warmed up; a time is the median of --reps launches, each between two device events on the stream (no host clock
inside the bracket); the three sides alternate in the one process; the select's outputs are compared byte for byte with the fresh
build's; the shader clock is probed before and after.
mixed: the mixed forest of forest_ragged_bench.py (--trees trees, leaf counts log-uniform in [1, 4^7], seed 7), arity 4.
one4 / one2: one 4^12-leaf tree alone in a forest (arity 2: 2^24 leaves).
Picks, per case: identity; 1 % of the trees dropped (the others keep their order); a random permutation; a merge of two halves (the
first and the second half of the trees built as two forests, gathered back in the original order).  A forest of one tree has no
tree to drop and one permutation: there the picks are the identity and the merge of two such trees, each from a forest of its own.
The copy moves the bytes the select moves — the used leaves, the used levels and the roots of the new forest — with three
hipMemcpyDtoDAsync calls; `rate_over_copy` is the select's bytes per second over the copy's, that is copy time over select time.
Prints one line per pick, writes them to --out, and prints a JSON summary last."""
import argparse
import ctypes
import json
import os

import numpy as np

import _common as C
from _common import ROOT
from testsupport import treeshape as TS


def _hip_runtime():
    """the HIP runtime the process runs on (torch's bundled copy once torch is imported), for hipMemcpyDtoDAsync"""
    import torch
    bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(bundled if os.path.exists(bundled) else "libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    return hip


class Forest:
    """a forest of random leaves built on the device with its tree-major levels: the tuple the select takes"""

    def __init__(self, ctx, arity, sizes):
        import torch
        from poseidon252_amd import merkle as M
        sizes = np.asarray(sizes, dtype=np.int64)
        self.sizes, self.T, self.n_leaves, self.max_leaves = sizes, len(sizes), int(sizes.sum()), int(sizes.max())
        self.d_off = C.dev(TS.offsets(sizes, dtype=np.int64))
        self.d = torch.randint(0, 1 << 60, (self.n_leaves, 4), dtype=torch.int64, device="cuda:0")
        self.lv = torch.empty((TS.levels_bound(self.n_leaves, self.T, self.max_leaves, arity), 4), dtype=torch.int64, device="cuda:0")
        self.roots = torch.empty((self.T, 4), dtype=torch.int64, device="cuda:0")
        ctx.merkle_forest_ragged_device(M.merkle4_tag() if arity == 4 else M.merkle2_tag(), self.d, self.d_off, self.T, self.max_leaves, self.roots,
                                        self.lv, arity=arity)

    def view(self):
        return (self.d, self.d_off, self.T, self.max_leaves, self.lv, self.roots)


class Pick:
    """one select — sources, pick list, exact-sized output buffers — with its fresh build and its copy of the same bytes"""

    def __init__(self, ctx, hip, arity, a, b, pick):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.hip, self.arity, self.a, self.b = ctx, hip, arity, a, b
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        pick = np.asarray(pick, dtype=np.int64)
        sizes = np.concatenate([a.sizes, b.sizes]) if b is not None else a.sizes
        new = sizes[pick]
        self.n_pick, self.leaves, self.max_leaves = len(pick), int(new.sum()), max(a.max_leaves, b.max_leaves if b is not None else 0)
        self.levels_used = int(TS.levels_len(new, arity).sum())
        self.bytes = 32 * (self.leaves + self.levels_used + self.n_pick)
        self.d_pick = C.dev(pick)
        cap = TS.levels_bound(self.leaves, self.n_pick, self.max_leaves, arity)
        new3 = lambda: (torch.zeros((self.leaves, 4), dtype=torch.int64, device="cuda:0"),  # noqa: E731
                        torch.zeros((max(cap, 1), 4), dtype=torch.int64, device="cuda:0"),
                        torch.zeros((self.n_pick, 4), dtype=torch.int64, device="cuda:0"))
        self.s_leaves, self.s_lv, self.s_roots = new3()
        self.c_leaves, self.f_lv, self.f_roots = new3()  # the copy's leaves; the fresh build's levels and roots
        self.c_lv, self.c_roots = torch.empty_like(self.s_lv), torch.empty_like(self.s_roots)
        self.s_off = torch.zeros(self.n_pick + 1, dtype=torch.int64, device="cuda:0")
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")

    def select(self, count=False):
        call = self.ctx.merkle4_forest_ragged_select_device if self.arity == 4 else self.ctx.merkle2_forest_ragged_select_device
        call(self.a.view(), self.b.view() if self.b is not None else None, self.d_pick, self.n_pick, self.s_leaves, self.s_off, self.s_lv, self.s_roots,
             self.bad if count else None)

    def rebuild(self):
        """the fresh build of the new forest, from the select's own leaves and offsets"""
        self.ctx.merkle_forest_ragged_device(self.tag, self.s_leaves, self.s_off, self.n_pick, self.max_leaves, self.f_roots, self.f_lv, arity=self.arity)

    def copy(self):
        import torch
        st = torch.cuda.current_stream().cuda_stream
        for dst, src, n in ((self.c_leaves, self.s_leaves, self.leaves), (self.c_lv, self.s_lv, self.levels_used), (self.c_roots, self.s_roots, self.n_pick)):
            if n and self.hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), n * 32, st) != 0:
                raise RuntimeError("hipMemcpyDtoDAsync failed")

    def outputs_equal(self):
        import torch
        torch.cuda.synchronize()
        return int(self.bad) == 0 and int(self.s_off[-1]) == self.leaves and bool(torch.equal(self.s_roots, self.f_roots)) and \
            bool(torch.equal(self.s_lv, self.f_lv))


def _measure(p, reps):
    import torch
    p.select(count=True)
    p.rebuild()
    p.copy()
    same = p.outputs_equal()
    t_sel, t_build, t_copy = C.alternate([p.select, p.rebuild, p.copy], reps, C.event_ms)
    torch.cuda.synchronize()
    return {"trees": p.n_pick, "leaves": p.leaves, "bytes": p.bytes, "select_ms": t_sel, "rebuild_ms": t_build, "copy_ms": t_copy,
            "rebuild_over_select": t_build / t_sel, "select_gbs": 2 * p.bytes / t_sel / 1e6, "copy_gbs": 2 * p.bytes / t_copy / 1e6,
            "rate_over_copy": t_copy / t_sel, "outputs_equal": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trees", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--cases", default="mixed,one4,one2", help="which of mixed, one4, one2 to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_select.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 / 2^16-leaf trees, 2,000 trees): a check of the tool, not a measurement")
    a = ap.parse_args()
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    hip = _hip_runtime()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cases = [c for c in a.cases.split(",") if c]
    res = {"reps": a.reps, "clock_mhz_before": C.clock_mhz(ctx), "cases": {}}
    say("python bench_tools/forest_select_bench.py --reps %d --cases %s%s   shader clock before: %s MHz"
        % (a.reps, a.cases, " --quick" if a.quick else "", res["clock_mhz_before"]))

    def run(case, name, arity, fa, fb, pick):
        p = Pick(ctx, hip, arity, fa, fb, pick)
        r = _measure(p, a.reps)
        res["cases"][case]["picks"][name] = r
        say("%s arity %d, %s: %d trees, %d leaves, %d bytes: select %.3f ms = %.0f GB/s read + written  fresh build %.3f ms  build/select %.1f  "
            "hipMemcpyDtoDAsync of the same bytes %.3f ms = %.0f GB/s  select rate / copy rate %.2f  outputs equal %s"
            % (case, arity, name, r["trees"], r["leaves"], r["bytes"], r["select_ms"], r["select_gbs"], r["rebuild_ms"], r["rebuild_over_select"],
               r["copy_ms"], r["copy_gbs"], r["rate_over_copy"], r["outputs_equal"]))
        del p
        torch.cuda.empty_cache()

    rng = np.random.default_rng(a.seed)
    if "mixed" in cases:
        top = 4 ** 7
        n_trees = 2000 if a.quick else a.trees
        sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), n_trees))).astype(np.int64).clip(1, top)
        res["cases"]["mixed"] = {"arity": 4, "trees": n_trees, "leaves": int(sizes.sum()), "picks": {}}
        f = Forest(ctx, 4, sizes)
        run("mixed", "identity", 4, f, None, np.arange(n_trees))
        run("mixed", "1 % dropped", 4, f, None, np.flatnonzero(rng.random(n_trees) >= 0.01))
        run("mixed", "permutation", 4, f, None, rng.permutation(n_trees))
        del f
        torch.cuda.empty_cache()
        half = n_trees // 2
        fa, fb = Forest(ctx, 4, sizes[:half]), Forest(ctx, 4, sizes[half:])
        run("mixed", "merge of two halves", 4, fa, fb, np.arange(n_trees))
        del fa, fb
        torch.cuda.empty_cache()
    for case, arity, n in (("one4", 4, 4 ** 8 if a.quick else 4 ** 12), ("one2", 2, 2 ** 16 if a.quick else 2 ** 24)):
        if case not in cases:
            continue
        res["cases"][case] = {"arity": arity, "trees": 1, "leaves": n, "picks": {}}
        fa = Forest(ctx, arity, [n])
        run(case, "identity", arity, fa, None, [0])
        fb = Forest(ctx, arity, [n])
        run(case, "merge of two halves", arity, fa, fb, [0, 1])
        del fa, fb
        torch.cuda.empty_cache()
    res["clock_mhz_after"] = C.clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
