"""Every message shape of tests/shapecases.py through the sponge, cipher and opening kernels on the GPU: every (in_len, out_len) with
in_len 1 .. 18 and 40 .. 44 in three layouts, plain and truncated; every cipher length 1 .. 18 and 41 .. 43 in both variants, with
a tampered copy that hits every element; every depth 0 .. 13, 16, 20 of both arities in three layouts.  Every output row is compared
with the oracle, and the ragged calls on one length or depth must give the bytes of the fixed-shape calls.

The tests of this process run the lane-group kernels (n = 70).  The one-lane, whole-line and truncating builds are selected by
P252_COOP_MAX_NODES=0, which the library reads once per process: children (tests/helpers/shape_sweep_driver.py, one per family so
that each stays within a few seconds) run the same sweeps at n = 323, children with P252_LINE_FETCH=0 as well must give the same
bytes block by block, and a kernel trace per environment shows that the sweeps reach the kernels the dispatch model of
shapecases.py predicts."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

import pytest

import edgecases as E
import shapecases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "helpers", "shape_sweep_driver.py")
ONE_LANE = {"P252_COOP_MAX_NODES": "0"}
BLOCK_BY_BLOCK = {"P252_COOP_MAX_NODES": "0", "P252_LINE_FETCH": "0"}
SPONGE_IN_LENS = sorted({i for i, _ in S.SPONGE_SHAPES})


def _default_environment():
    assert S.environment() == (16384, True), "these tests expect the library's default dispatch, not %r" % (S.environment(),)


# ---------------------------------------------------------------------------------------------- lane groups, this process
@pytest.mark.parametrize("in_len", SPONGE_IN_LENS)
def test_sponge_shapes_on_lane_groups(gpu_ctx, oracle_mod, in_len):
    """every out_len of the list at this in_len: k_sponge_coop and k_sponge_coop_trunc, and k_sponge_ragged_coop[_trunc] on n
    messages of this one length"""
    _default_environment()
    sw = S.Sweep(gpu_ctx, S.N_LANE_GROUPS)
    shapes = [s for s in S.SPONGE_SHAPES if s[0] == in_len]
    for i, o in shapes:
        S.sponge_shape(sw, i, o)
    want = {"k_sponge_coop", "k_sponge_coop_trunc"}
    if in_len in S.RAGGED_IN_LENS:
        S.sponge_ragged_equivalence(sw, in_len)
        want |= {"k_sponge_ragged_coop", "k_sponge_ragged_coop_trunc"}
    assert sw.kernels == want
    assert sw.rows == S.N_LANE_GROUPS * (len(shapes) * 6 + (2 if in_len in S.RAGGED_IN_LENS else 0))


@pytest.mark.parametrize("variant,length", S.CRYPT_CASES, ids=["%s-%d" % ("stream" if v == S.STREAM else "duplex", ln) for v, ln in S.CRYPT_CASES])
def test_cipher_shapes_on_lane_groups(gpu_ctx, oracle_mod, variant, length):
    """k_crypt_coop<false | true>: the ciphers, the messages back with every flag 1, and the tampered copy"""
    _default_environment()
    sw = S.Sweep(gpu_ctx, S.N_LANE_GROUPS)
    S.crypt_case(sw, variant, length)
    assert sw.kernels == {"k_crypt_coop"} and sw.rows == 3 * S.N_LANE_GROUPS


@pytest.mark.parametrize("arity,depth", S.PATH_CASES, ids=["arity%d-depth%d" % c for c in S.PATH_CASES])
def test_path_shapes_on_lane_groups(gpu_ctx, oracle_mod, arity, depth):
    """k_merkle4_path_coop / k_merkle2_path at small n in three layouts, and k_path_ragged at this one depth.  Depth 0 is ACCEPTED by
    p252_merkle{4,2}_path_batch_device (no sibling or position buffer is needed): the roots are the leaves, and this test pins it."""
    _default_environment()
    sw = S.Sweep(gpu_ctx, S.N_LANE_GROUPS)
    S.path_case(sw, arity, depth)
    assert sw.kernels == {"k_merkle4_path_coop" if arity == 4 else "k_merkle2_path", "k_path_ragged"}
    assert sw.rows == 4 * S.N_LANE_GROUPS


@pytest.mark.parametrize("arity", [4, 2])
def test_depth_zero_needs_no_sibling_or_position_buffer(gpu_ctx, oracle_mod, arity):
    """the fixed-depth re-hash at depth 0 with None for the siblings and positions: accepted, the leaves come back reduced"""
    import numpy as np
    import torch
    n = S.N_LANE_GROUPS
    leaves = oracle_mod.fill_random(0x55000 + arity, n)
    roots = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
    call = gpu_ctx.merkle4_path_batch_device if arity == 4 else gpu_ctx.merkle2_path_batch_device
    call(E._mtag(arity), E._dev(leaves), None, None, 0, roots, n)
    torch.cuda.synchronize()
    assert np.array_equal(E._host(roots), leaves)


# ---------------------------------------------------------------------------------------------- the other builds, in children
# a slice is (family, part): the sponge sweep runs as two children of every other shape, so that no child takes more than a few seconds
ONE_LANE_SLICES = [("sponge", (0, 2)), ("sponge", (1, 2)), ("crypt", S.WHOLE), ("paths", S.WHOLE)]
LINE_SLICES = [sl for sl in ONE_LANE_SLICES if sl[0] in ("sponge", "paths")]


def _slice_id(sl):
    return sl[0] if sl[1] == S.WHOLE else "%s-%d/%d" % ((sl[0],) + sl[1])


def _child(env, family, part):
    r = subprocess.run([sys.executable, DRIVER, "--check", "--n", str(S.N_ONE_LANE), "--families", family, "--part", "%d/%d" % part],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    print(r.stdout)
    assert report["shape_sweep"] == "ok" and report["checked"] and report["n"] == S.N_ONE_LANE and tuple(report["part"]) == part
    assert report["coop_max_nodes"] == 0 and report["line_fetch"] == (env.get("P252_LINE_FETCH") != "0")
    assert list(report["families"]) == [family]
    got = report["families"][family]  # an empty or a shortened sweep is no sweep
    assert got["rows"] == S.expected_rows(family, S.N_ONE_LANE, part) > 0
    assert set(got["kernels"]) == S.predicted_kernels(family, S.N_ONE_LANE, 0, report["line_fetch"], part)
    return got


def test_the_slices_are_the_whole_lists():
    for family in S.FAMILIES:
        parts = [part for f, part in ONE_LANE_SLICES if f == family]
        assert sum(S.expected_rows(family, S.N_ONE_LANE, part) for part in parts) == S.expected_rows(family, S.N_ONE_LANE)
        assert parts == [(i, len(parts)) for i in range(len(parts))]
        assert set().union(*[S.predicted_kernels(family, S.N_ONE_LANE, 0, True, part) for part in parts]) == ONE_LANE_KERNELS[family]
        for part in parts:  # and every child of the sponge sweep sees every build
            assert S.predicted_kernels(family, S.N_ONE_LANE, 0, True, part) == ONE_LANE_KERNELS[family]


_ONE_LANE_REPORTS = {}


def _one_lane(sl):
    """the report of the child with P252_COOP_MAX_NODES=0 that runs one slice at n = 323: started once.  If it failed, the tests that
    need it fail too and start nothing else."""
    if sl not in _ONE_LANE_REPORTS:
        _ONE_LANE_REPORTS[sl] = None
        _ONE_LANE_REPORTS[sl] = _child(ONE_LANE, *sl)
    if _ONE_LANE_REPORTS[sl] is None:
        pytest.fail("the one-lane child of %s failed: nothing else is started" % _slice_id(sl))
    return _ONE_LANE_REPORTS[sl]


ONE_LANE_KERNELS = {
    "sponge": {"k_sponge", "k_sponge_lines", "k_sponge_trunc", "k_sponge_lines_trunc", "k_sponge_ragged", "k_sponge_ragged_trunc"},
    "crypt": {"k_crypt"},
    "paths": {"k_merkle4_path", "k_merkle4_path_lines", "k_merkle2_path", "k_path_ragged"},
}


@pytest.mark.parametrize("sl", ONE_LANE_SLICES, ids=_slice_id)
def test_shapes_on_the_one_lane_kernels(sl):
    """k_sponge, k_sponge_lines and both _trunc forms, k_crypt<false | true>, k_merkle4_path, k_merkle4_path_lines, k_merkle2_path: every
    row of every shape equals the oracle's (the child checks; its report counts the rows)"""
    assert set(_one_lane(sl)["kernels"]) == ONE_LANE_KERNELS[sl[0]]


@pytest.mark.parametrize("sl", LINE_SLICES, ids=_slice_id)
def test_block_by_block_gives_the_bytes_of_whole_lines(sl):
    """a child with P252_LINE_FETCH=0 as well: the sponge and opening sweeps on k_sponge[_trunc] and k_merkle4_path in EVERY layout —
    the same SHA-256 over all outputs as with whole-line fetches"""
    first = _one_lane(sl)
    report = _child(BLOCK_BY_BLOCK, *sl)
    assert report["sha256"] == first["sha256"]
    assert not any("lines" in k for k in report["kernels"]) and any("lines" in k for k in first["kernels"])


# ---------------------------------------------------------------------------------------------- reach
ENVIRONMENTS = {
    "default": ({}, S.N_LANE_GROUPS, S.FAMILIES, (16384, True)),
    "one_lane": (ONE_LANE, S.N_ONE_LANE, S.FAMILIES, (0, True)),
    "block_by_block": (BLOCK_BY_BLOCK, S.N_ONE_LANE, ("sponge", "paths"), (0, False)),
}


@pytest.mark.parametrize("which", sorted(ENVIRONMENTS))
def test_the_sweeps_reach_the_kernels_the_model_predicts(tmp_path, which):
    """dispatch thresholds move; a sweep that lands on another kernel no longer tests the one it names.  The GPU side of the sweeps
    under the kernel tracer, once per environment: every kernel the dispatch model predicts is among the traced ones."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        pytest.skip("rocprofv3 not on this box")
    switched, n, families, (coop_max, line_fetch) = ENVIRONMENTS[which]
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR="/tmp")
    env.update(switched)
    program = [sys.executable, DRIVER, "--n", str(n), "--families", ",".join(families)]
    r = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "kt", "--"] + program,
                       cwd="/tmp", env=env, capture_output=True, timeout=300)
    files = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 and not files:  # the PROFILER could not run here (no counters / permissions): nothing was learnt about the library
        pytest.skip("rocprofv3 could not trace on this box: " + r.stderr.decode()[-300:])
    assert r.returncode == 0 and files, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    traced = sorted({row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))})
    expected = sorted({k for family in families for k in S.predicted_kernels(family, n, coop_max, line_fetch)})
    assert len(expected) >= 5
    missing = [k for k in expected if not E.kernel_in_trace(k, traced)]
    assert not missing, "kernels the sweep did not reach: %s\ntraced: %s" % (missing, [t for t in traced if "p252" in t])
    if which == "block_by_block":  # and the switch is a switch
        assert not any(E.kernel_in_trace(k, traced) for k in ("k_sponge_lines", "k_sponge_lines_trunc", "k_merkle4_path_lines"))
