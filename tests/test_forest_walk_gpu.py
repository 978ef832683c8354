"""One ragged Merkle forest carried through long mixed sequences of forest calls on the GPU (tests/forestwalk.py): built once, then
updated, appended to, rolled back, reorganised, pruned, opened and proved again and again, each call reading what the call before it
wrote — against the oracle's single-tree builds and the numpy models of testsupport/ after EVERY step, never against the library itself
(tests/test_forest_walk_cpu.py checks the plans, the host model and that the runner's checks bite, without a GPU).  On the default
stream, on a side stream with p252_trim in the middle, on the one-lane kernels (a child process), and two walks interleaved on two
streams of one context."""
import json
import os
import subprocess
import sys
import time

import pytest

import forestwalk as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLANS = {}


def _plan(profile, arity):
    if (profile, arity) not in _PLANS:
        _PLANS[(profile, arity)] = W.plan(profile, arity)
    return _PLANS[(profile, arity)]


@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("profile", ["small", "wide"])
def test_walk_matches_the_oracle(gpu_ctx, oracle_mod, profile, arity):
    P = _plan(profile, arity)
    t0 = time.perf_counter()
    w = W.run(P, W.GpuBackend(gpu_ctx))
    seconds = time.perf_counter() - t0
    shares = w.fresh_only[1:-1]  # (per step; the build before them and the final state after them: the oracle on every tree at the end)
    print("walk %s arity %d: %d steps in %.2f s; share of trees per step that the fresh build alone covers: %s"
          % (profile, arity, len(P.steps), seconds, " ".join("%.3f" % x for x in shares)))
    assert len(w.fresh_only) == len(P.steps) + 2 and w.fresh_only[-1] == 0.0  # no step unchecked, the last state against the oracle on every tree
    assert profile == "wide" or not any(w.fresh_only)


def test_walk_on_a_side_stream_with_a_trim_in_the_middle(gpu_ctx, oracle_mod):
    """the scratch of the side stream regrows from nothing under a call other than the build"""
    import torch
    P = _plan("small", 4)
    mid = [i for i, s in enumerate(P.steps, 1) if s["kind"] == "reorg"][0]
    trimmed = []

    def before(i):
        if i == mid:
            torch.cuda.synchronize()
            gpu_ctx.trim()
            trimmed.append(i)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = W.run(P, W.GpuBackend(gpu_ctx), before_step=before)
    torch.cuda.synchronize()
    assert trimmed == [mid] and len(w.fresh_only) == len(P.steps) + 2


def test_small_walk_on_the_one_lane_kernels():
    """P252_COOP_MAX_NODES=0 (read once per process): every digest launch of both small walks on k_fr_digest / k_fu_digest / k_mp_digest"""
    env = dict(os.environ, P252_COOP_MAX_NODES="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "forest_walk_driver.py"), "--profile", "small", "--arities", "4,2"],
                         capture_output=True, env=env, timeout=300)
    text = out.stdout.decode() + out.stderr.decode()
    assert out.returncode == 0, text[-4000:]
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    print(text)
    assert res["forest_walk"] == "ok" and res["checked"] is True and res["coop_max_nodes"] == "0"
    assert res["steps"] == {"4": len(_plan("small", 4).steps), "2": len(_plan("small", 2).steps)}


def test_walks_interleaved_on_two_streams_of_one_context(gpu_ctx, oracle_mod):
    """the arity-4 and the arity-2 walk advance alternately, one step each, on two streams; the two calls of a pair (and their read
    phases) are launched without a host synchronisation between them: the per-stream scratch keeps them apart"""
    import torch
    plans = [_plan("small", 4), _plan("small", 2)]
    assert len(plans[0].steps) == len(plans[1].steps)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    walks = [W.Walk(p, W.GpuBackend(gpu_ctx)) for p in plans]
    for w, s in zip(walks, streams):
        with torch.cuda.stream(s):
            w.build()
    for i in range(1, len(plans[0].steps) + 1):
        for w, s in zip(walks, streams):
            with torch.cuda.stream(s):
                w.prepare(i)
        torch.cuda.synchronize()
        for w, s in zip(walks, streams):  # library calls and device-side copies only
            with torch.cuda.stream(s):
                w.launch(i)
        torch.cuda.synchronize()
        for w, s in zip(walks, streams):
            with torch.cuda.stream(s):
                w.check(i)
    for w, s in zip(walks, streams):
        with torch.cuda.stream(s):
            w.final()
    assert all(len(w.fresh_only) == len(p.steps) + 2 for w, p in zip(walks, plans))
