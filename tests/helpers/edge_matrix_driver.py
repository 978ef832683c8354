"""Driver of tests/test_edge_values_gpu.py — runs rows of the edge-value matrix (tests/edgecases.py) in a process of its own:

  python tests/helpers/edge_matrix_driver.py [--check] [--rows name,name,...]

Without --check: the GPU side of every row once, nothing compared — what the kernel tracer runs, to see which kernels the rows'
sizes reach.  With --check: the rows against the oracle, as the tests do in their own process — for the children that set
P252_TREE_PAD_LANES / P252_COOP_MAX_NODES, which the library reads once per process.  Prints one line per row, then a JSON line."""
import argparse
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edgecases as E  # noqa: E402
import poseidon252_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare every row with the oracle")
    ap.add_argument("--rows", default="", help="comma-separated row names (default: every row)")
    ap.add_argument("--keep-going", action="store_true", help="after a row that differs from the oracle, run the rows that follow")
    a = ap.parse_args()
    rows = [E.BY_NAME[n] for n in a.rows.split(",")] if a.rows else E.ROWS
    run = E.Run(P.Context(0), check=a.check)
    seconds = {}
    failed = []
    for row in rows:
        try:
            seconds[row.name] = round(row(run), 3)
        except (AssertionError, ValueError, TypeError, IndexError, KeyError, AttributeError):
            # a mismatch or a refused call: the next row still runs with --keep-going (a device error always ends the run)
            if not a.keep_going:
                raise
            failed.append(row.name)
            print("ROW %-26s FAILED:\n%s" % (row.name, traceback.format_exc(limit=6)), flush=True)
            continue
        print("ROW %-26s %7.3f s  %s" % (row.name, seconds[row.name], " ".join(row.kernels)), flush=True)
    print(json.dumps({"edge_matrix": "failed" if failed else "ok", "checked": a.check, "rows": seconds, "failed": failed}))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
