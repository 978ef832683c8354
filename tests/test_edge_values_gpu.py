"""Edge values through EVERY hashing entry point on the GPU (the matrix of tests/edgecases.py): inputs from edge_scalars — 0, 1,
p - 1, limb patterns at and above p up to 2^256 - 1, saturated 29- and 32-bit digits, mixed with random scalars — go to the GPU
raw and to the oracle reduced mod p; the outputs are the same bytes, every one canonical.  What is hashed, absorbed, added or
subtracted counts mod p; what is compared (the stored MAC, the expected root) is compared as its 32 bytes: an unreduced twin of
a leaf, a sibling or a cipher element changes nothing, MAC + p and root + p are refused.

Each row's sizes select one kernel under the default environment (its name is in the row); the rows of lane-group size run again
on the one-lane kernels, the two trees again on k_merkle4_pad, each in a child with the environment that selects them; and a
kernel trace of the whole matrix shows that the rows still reach the kernels they name."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

import pytest

import edgecases as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "helpers", "edge_matrix_driver.py")


@pytest.mark.parametrize("row", E.ROWS, ids=[r.name for r in E.ROWS])
def test_row_matches_the_oracle(gpu_ctx, oracle_mod, row):
    seconds = row(E.Run(gpu_ctx, check=True))
    print("%s: %.2f s (%s)" % (row.name, seconds, ", ".join(row.kernels)))


def _child(env, names):
    r = subprocess.run([sys.executable, DRIVER, "--check", "--rows", ",".join(names)], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report["edge_matrix"] == "ok" and report["checked"] and sorted(report["rows"]) == sorted(names)
    print(r.stdout)


def test_trees_on_the_padded_narrow_level_kernel():
    """P252_TREE_PAD_LANES=65538 (read once per process: a child, one for both arities): level 1 of both trees, 16,386 nodes, runs
    k_merkle4_pad"""
    env, names, _ = E.CHILDREN["pad"]
    _child(env, names)


def test_lane_group_rows_on_the_one_lane_kernels():
    """P252_COOP_MAX_NODES=0: the same inputs of every lane-group-sized row through the one-lane kernels at small n"""
    env, names, _ = E.CHILDREN["one_lane"]
    _child(env, names)


@pytest.mark.parametrize("which", ["default", "pad", "one_lane"])
def test_the_matrix_reaches_the_kernels_it_names(tmp_path, which):
    """dispatch thresholds move; a row that lands on another kernel no longer tests the one it names.  The GPU side of every
    default-environment row under the kernel tracer (and of each child's rows under its environment): every kernel the rows name
    is among the traced ones, and every hashing kernel of csrc/*.hip is named by a row or by one of the two children."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        pytest.skip("rocprofv3 not on this box")
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR="/tmp")
    program = [sys.executable, DRIVER]
    expected = sorted({k for row in E.ROWS for k in row.kernels})
    if which != "default":
        switched, names, expected = E.CHILDREN[which]
        env.update(switched)
        program += ["--rows", ",".join(names)]
    r = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "kt", "--"] + program,
                       cwd="/tmp", env=env, capture_output=True, timeout=600)
    files = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 and not files:  # the PROFILER could not run here (no counters / permissions): nothing was learnt about the library
        pytest.skip("rocprofv3 could not trace on this box: " + r.stderr.decode()[-300:])
    assert r.returncode == 0 and files, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    traced = sorted({row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))})
    missing = [k for k in expected if not E.kernel_in_trace(k, traced)]
    assert not missing, "kernels no row reached: %s\ntraced: %s" % (missing, [n for n in traced if "p252" in n])
    unnamed = E.hashing_kernels() - E.named_kernels()
    assert not unnamed, "hashing kernels that no row names: %s" % sorted(unnamed)
