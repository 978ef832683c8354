"""Driver of tests/test_soundness_gpu.py — puts one batch of changed openings to p252_merkle{4,2}_verify_batch_device or
_forest_ragged_verify_device, in this process (run_sweep) or in a process of its own:

  python tests/helpers/soundness_driver.py IN.npz OUT.npz

for the children that set P252_COOP_MAX_NODES / P252_LINE_FETCH / P252_RAGGED_SORT, which the library reads once per process.  IN holds
batches as tests/soundcases.py makes them (job below; pack puts several into one file); OUT for each the verdict vectors and the path
kernel the dispatch model (shapecases) expects under this process's environment.  Nothing is compared here: the test holds the model's verdicts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TAIL = 3  # canary bytes behind every verdict vector


def job(sw, arity, fixed, chunk=0):
    """the arrays of one sweep (a dict of soundcases._swept): the batch, the good openings' count, the changed roots"""
    B = sw["batch"]
    return dict(arity=arity, fixed=int(fixed), chunk=chunk, stride=B["stride"], leaves=B["leaves"], sib=B["sib"], pos=B["pos"], dep=B["dep"], tid=B["tid"],
                roots=B["roots"], n_good=len(sw["good"]["dep"]), alt_roots=np.array([r for _, r, _ in sw["roots"]]))


def _verify(ctx, J, rows, roots):
    """the first `rows` openings of the batch against `roots` -> ok (rows,) uint8; a fixed-depth batch goes in calls of at most `chunk`"""
    import torch
    from helpers.forest import _tag, _torch
    arity, D = int(J["arity"]), int(J["stride"])
    leaves, sib, pos = _torch(J["leaves"][:rows]), _torch(J["sib"][:rows]), _torch(J["pos"][:rows])
    ok = torch.full((rows + TAIL,), 7, dtype=torch.uint8, device="cuda:0")
    if int(J["fixed"]):
        d_root, step = _torch(roots[0]), int(J["chunk"]) or rows
        for a in range(0, rows, step):
            b = min(rows, a + step)
            ctx.merkle_verify_batch_device(_tag(arity), leaves[a:b], sib[a:b], pos[a:b], D, d_root, ok[a:b], b - a, arity=arity)
    else:
        ctx.merkle_forest_ragged_verify_device(_tag(arity), leaves, sib, pos, _torch(J["dep"][:rows]), D, _torch(J["tid"][:rows]), _torch(roots),
                                               len(roots), ok[:rows], rows, arity=arity)
    torch.cuda.synchronize()
    assert bool((ok[rows:] == 7).all()), "a verdict was written past the batch"
    return ok[:rows].cpu().numpy()


def run_sweep(ctx, J):
    """-> dict(ok = the whole batch against the good roots, alt = the good openings against each set of changed roots, after = the good
    openings against the good roots once more, kernel = the path kernel expected for the largest call)"""
    import shapecases as SC
    n, good = len(J["dep"]), int(J["n_good"])
    out = dict(ok=_verify(ctx, J, n, J["roots"]), alt=np.array([_verify(ctx, J, good, r) for r in J["alt_roots"]]))
    out["after"] = _verify(ctx, J, good, J["roots"])
    coop_max, line_fetch = SC.environment()
    per_call = min(n, int(J["chunk"]) or n)
    out["kernel"] = SC.path_kernel(int(J["arity"]), per_call, int(J["stride"]), "aligned", coop_max, line_fetch) if int(J["fixed"]) else "k_path_ragged"
    out["sorted"] = int(os.environ.get("P252_RAGGED_SORT", "1")[:1] != "0")
    return out


def pack(jobs):
    """several jobs (or their results) as the arrays of one .npz file"""
    return {"%d.%s" % (i, k): v for i, J in enumerate(jobs) for k, v in J.items()}


def unpack(z):
    jobs = {}
    for name in z.files:
        i, k = name.split(".", 1)
        jobs.setdefault(int(i), {})[k] = z[name]
    return [jobs[i] for i in sorted(jobs)]


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import poseidon252_amd as P
    src, dst = sys.argv[1:3]
    with np.load(src) as z:
        jobs = unpack(z)
    ctx = P.Context(0)
    np.savez(dst, **pack([run_sweep(ctx, J) for J in jobs]))
    print("done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
