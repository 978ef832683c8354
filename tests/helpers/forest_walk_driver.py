"""Driver of tests/test_forest_walk_gpu.py — runs forest walks (tests/forestwalk.py) in a process of its own:

  python tests/helpers/forest_walk_driver.py [--profile small] [--arities 4,2]

for the child that sets P252_COOP_MAX_NODES, which the library reads once per process.  Every walk runs with check=True, as the tests
run it in their own process.  Prints one line per walk, then a JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forestwalk as W  # noqa: E402
import poseidon252_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--profile", default="small")
    ap.add_argument("--arities", default="4,2")
    a = ap.parse_args()
    backend = W.GpuBackend(P.Context(0))
    seconds, steps = {}, {}
    for arity in (int(x) for x in a.arities.split(",")):
        plan = W.plan(a.profile, arity)
        t0 = time.perf_counter()
        W.run(plan, backend, check=True)  # (a mismatch raises: the process ends with a traceback and a non-zero status)
        seconds[str(arity)], steps[str(arity)] = round(time.perf_counter() - t0, 3), len(plan.steps)
        print("WALK %s arity %d: %d steps %7.3f s" % (a.profile, arity, len(plan.steps), seconds[str(arity)]), flush=True)
    print(json.dumps({"forest_walk": "ok", "checked": True, "profile": a.profile, "coop_max_nodes": os.environ.get("P252_COOP_MAX_NODES"),
                      "steps": steps, "seconds": seconds}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
