"""Driver of tests/test_shape_sweep_gpu.py — runs the shape sweeps (tests/shapecases.py) in a process of its own:

  python tests/helpers/shape_sweep_driver.py [--check] [--n 323] [--families sponge,crypt,paths] [--part i/k]

for the children that set P252_COOP_MAX_NODES / P252_LINE_FETCH, which the library reads once per process.  With --check: every
output row against the oracle.  Without: the GPU side alone, nothing compared — what the kernel tracer runs.  Prints one line per
family, then a JSON line: per family the rows compared, a SHA-256 over every output, and the kernels the dispatch model expects."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shapecases as S  # noqa: E402
import poseidon252_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare every output row with the oracle")
    ap.add_argument("--n", type=int, default=S.N_ONE_LANE, help="messages per row")
    ap.add_argument("--families", default=",".join(S.FAMILIES), help="comma-separated: sponge, crypt, paths")
    ap.add_argument("--part", default="0/1", help="i/k: every k-th case of each family's list from the i-th on (default: all)")
    a = ap.parse_args()
    part = tuple(int(v) for v in a.part.split("/"))
    assert len(part) == 2 and 0 <= part[0] < part[1]
    ctx = P.Context(0)
    report = {}
    for family in a.families.split(","):
        sw = S.Sweep(ctx, a.n, check=a.check)
        seconds = S.run_family(sw, family, part)  # (a mismatch raises: the process ends non-zero, and nothing more is started)
        report[family] = {"rows": sw.rows, "sha256": sw.sha.hexdigest(), "kernels": sorted(sw.kernels), "seconds": round(seconds, 3)}
        print("FAMILY %-7s n=%d %8d rows %7.3f s  %s" % (family, a.n, sw.rows, seconds, " ".join(sorted(sw.kernels))), flush=True)
    coop_max, line_fetch = S.environment()
    print(json.dumps({"shape_sweep": "ok", "checked": a.check, "n": a.n, "coop_max_nodes": coop_max, "line_fetch": line_fetch,
                      "part": list(part), "families": report}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
