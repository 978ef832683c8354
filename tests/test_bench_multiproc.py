"""bench.py contract checks on the GPU box: the single JSON line at N=1, and the N>1 code path
(launched exactly as the driver launches it, via torch.distributed.run) exercised with 2 ranks that
SHARE the one available GPU and use gloo for the collectives (test-only env switches; on an 8-GPU
node the driver runs it with the default nccl = RCCL backend, one rank per GPU)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


LINE_BUDGET = 6000  # the driver keeps an 8 KB tail of stdout; round 4's 26 KB line could not be parsed


def _scalars_only(obj, depth=0):
    """the printed line nests at most: line -> roofline / config / cpu_baseline / secondary -> workload -> scalars (+ reference_cargo_bench)"""
    for k, v in obj.items():
        if isinstance(v, dict):
            assert depth < 3, k
            _scalars_only(v, depth + 1)
        else:
            assert v is None or isinstance(v, (bool, int, float, str)), (k, v)


def _one_json_line(out, want_detail=False):
    """the ONE line on stdout: bounded in length, scalars only; the full record (nested models, per-rank arrays, sources, notes) is in
    the side file the line names"""
    lines = [l for l in out.decode().splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.decode()
    assert len(lines[0]) < LINE_BUDGET, len(lines[0])
    d = json.loads(lines[0])
    _scalars_only(d)
    assert "line_trimmed" not in d and d["detail_file"] == "bench_detail.json"
    if not want_detail:
        return d
    full = json.load(open(os.path.join(ROOT, d["detail_file"])))
    assert full["value"] == pytest.approx(d["value"], rel=1e-7) and full["n_gpus"] == d["n_gpus"] and full["config"]["workload"].startswith(d["config"]["workload"].rstrip("."))
    for k, v in d["roofline"].items():  # the line's roofline = the record's top-level scalars
        assert full["roofline"][k] == (pytest.approx(v, rel=1e-6) if isinstance(v, float) else v), k
    for key, w in d.get("secondary", {}).items():
        fw = full["secondary"][key]
        assert fw["value"] == pytest.approx(w["value"], rel=1e-7) and fw["roofline"]["kernel"] == w["kernel"] and fw["self_consistency_ok"] == w["self_consistency_ok"]
        assert w["frac"] == pytest.approx(fw["roofline"]["frac"], rel=1e-6)
    return d, full


def test_bench_single_gpu_json_line(gpu_ctx):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                                   "--log2n", "16", "--no-cpu-baseline", "--no-secondary"], cwd=ROOT, timeout=600)
    d, full = _one_json_line(out, want_detail=True)
    for k in REQUIRED:
        assert k in d and k in full, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["self_consistency_ok"] is True
    assert d["value"] > 1e6 and d["scaling"] == "weak" and d["vs_baseline"] is None
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic"):  # the contract's roofline keys, on the line itself
        assert k in d["roofline"], k
    assert d["roofline"]["frac"] == pytest.approx(d["roofline"]["achieved"] / d["roofline"]["peak"], rel=1e-5)
    r = full["roofline"]
    assert r["hbm"]["frac"] < 0.05 and r["hbm_frac"] == r["hbm"]["frac"]
    _check_roofline_scalars(r)
    _check_clock(r)
    assert "secondary" not in d  # (a plain run: only a --full line carries them, see the next test)


def _check_roofline_scalars(r):
    """the top-level scalars of `roofline` (all the driver's record keeps) carry the HARDWARE fraction —
    multiply-adds the kernel actually issues / the VALU issue peak, at most 1 — and its companions; SURVEY §8d's
    256,000-MAC pricing of the reference schedule is kept under its own name"""
    for k in ("achieved", "peak", "frac", "frac_at_measured_clock", "frac_valu_issue", "macs_per_perm_executed", "clock_ghz_measured",
              "frac_reference_schedule", "achieved_reference_schedule", "launch_ms_mean", "units_per_launch", "traffic_algorithmic_bytes"):
        assert isinstance(r[k], (int, float)) and not isinstance(r[k], bool), (k, r[k])
    assert "traffic" in r and "traffic_ratio" in r and (r["traffic"] is None or isinstance(r["traffic"], float))
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"]) and 0 < r["frac"] <= 1.0 and r["frac_at_measured_clock"] <= 1.0
    assert r["achieved"] == pytest.approx(r["macs_per_perm_executed"] * r["units_per_launch"] / (r["launch_ms_mean"] * 1e-3) / 1e12, rel=1e-9)
    assert r["frac_reference_schedule"] == pytest.approx(r["achieved_reference_schedule"] / r["peak"])
    assert r["achieved_reference_schedule"] == pytest.approx(256000 * r["units_per_launch"] / (r["launch_ms_mean"] * 1e-3) / 1e12, rel=1e-9)
    assert r["frac"] == r["executed"]["frac"] and r["frac_valu_issue"] == r["valu_issue"]["frac"] and r["frac"] < r["frac_valu_issue"] <= 1.0
    assert r["clock_ghz_measured"] == r["clock"]["ghz_measured"]
    assert r["frac_at_measured_clock"] == pytest.approx(r["frac"] * 2.4 / r["clock_ghz_measured"], rel=1e-6)


def _check_clock(r):
    """the shader clock measured inside the run, and the fractions at it"""
    c = r["clock"]
    assert c["before"] and c["after"], c
    for probe in (c["before"], c["after"]):
        assert 1.0 < probe["shader_ghz"] < 2.6 and probe["interval_us"] > 100, probe
    assert c["ghz_measured"] == pytest.approx((c["before"]["shader_ghz"] + c["after"]["shader_ghz"]) / 2)
    e = r["executed"]
    assert e["frac_at_measured_clock"] == pytest.approx(e["frac"] * 2.4 / c["ghz_measured"], rel=1e-6)
    assert r["valu_issue"]["frac_at_measured_clock"] == pytest.approx(r["valu_issue"]["frac"] * 2.4 / c["ghz_measured"], rel=1e-6)


def test_bench_default_line_carries_the_secondary_workloads(gpu_ctx):
    """one command times every BASELINE config (with --full) — configs[1] as the primary keys, the tree
    (configs[2]; configs[4] at 8 ranks) and the 42 -> 5 sponge (configs[3]) under "secondary", each with its own
    self-consistency check, roofline, measured clock and (N = 1) oracle check of a sample.  Scaled down here."""
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--log2n", "15",
                                   "--secondary-log2n", "14", "--full"], cwd=ROOT, timeout=900, stderr=subprocess.DEVNULL)
    line, d = _one_json_line(out, want_detail=True)  # (the length budget and scalars-only shape are asserted on the real line in there)
    for k in REQUIRED + ["cpu_baseline", "secondary"]:
        assert k in d and k in line, k
    assert sorted(line["secondary"]) == sorted(d["secondary"]) and line["cpu_baseline"]["parity_sample_ok"] is True
    # (the cpu_baseline leg — ~25 s of oracle time on the host cores — runs in THIS test only: it times the oracle and verifies a sample
    # of the GPU output of the primary and of every secondary, the openings' sample kind included; until round 5 two more tests paid for it)
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] >= 1 and line["cpu_baseline"]["value"] > 1e3
    for k in ("value", "unit", "cores", "kind", "sample"):  # the contract's cpu_baseline keys, on the line itself
        assert line["cpu_baseline"][k] is not None, k
    assert line["cpu_baseline"]["reference_cargo_bench"]["available"] in (True, False)
    for w in line["secondary"].values():
        assert w["self_consistency_ok"] is True and w["parity_sample_ok"] is True and 0 < w["frac"] <= 1 and w["value"] > 1e6
    assert "BASELINE configs[1]" in d["config"]["workload"] and d["self_consistency_ok"] is True
    sec = d["secondary"]
    assert sorted(sec) == ["encrypt", "extract", "forest", "openings", "sponge42", "tree"]
    x = sec.pop("extract")  # the HBM-bound workload: openings extracted from a stored tree (data movement), the contract's "hbm" shape
    assert x["roofline"]["bound"] == "hbm" and x["roofline"]["kernel"] == "k_merkle4_openings" and x["unit"] == "opening levels/s"
    assert x["roofline"]["frac"] == pytest.approx(x["roofline"]["achieved"] / 8000.0) and 0 < x["roofline"]["frac"] < 1
    assert x["units_per_gpu_per_step"] == (1 << 14) * 9 and x["self_consistency_ok"] is True and x["parity_sample_ok"] is True  # 2^18-leaf tree: depth 9
    f = sec["forest"]  # 2^18 leaves as 64 trees of 4^6 leaves: one launch per level across all trees
    assert "forest of 64 independent arity-4 Merkle trees of 4^6 leaves" in f["workload"] and f["units_per_gpu_per_step"] == 64 * 1365
    assert f["self_consistency_ok"] is True and f["parity_sample_ok"] is True and f["roofline"]["kernel"] == "k_merkle4"
    t, s = sec["tree"], sec["sponge42"]
    for w, kern, units in ((sec["openings"], "k_merkle4_path_lines", 12 << 14), (sec["encrypt"], "k_crypt", 2 << 14)):
        assert w["roofline"]["kernel"] == kern and w["units_per_gpu_per_step"] == units
        assert w["self_consistency_ok"] is True and w["parity_sample_ok"] is True and w["value"] > 1e6
    assert "2^18-leaf arity-4 Merkle tree" in t["workload"]
    assert t["units_per_gpu_per_step"] == (4 ** 9 - 1) // 3  # 4^9 leaves: 65536 + 16384 + ... + 4 + 1 = 87381 nodes
    assert s["units_per_gpu_per_step"] == 12 << 14 and "42 scalars -> 5 outputs" in s["workload"]
    for w in (t, s):
        assert w["self_consistency_ok"] is True and w["parity_sample_ok"] is True and w["n_gpus"] == 1 and w["ranks"] == 1
        assert w["value"] == pytest.approx(w["units_per_gpu_per_step"] * w["steps"] / (w["ms_per_step"] * w["steps"] * 1e-3), rel=1e-6)
        assert w["steps"] == 3 and w["roofline"]["executed"]["frac"] > 0 and w["roofline"]["launch_ms_mean"] > 0
        _check_clock(w["roofline"])
        _check_roofline_scalars(w["roofline"])
        assert w["ms_per_step_rank_min"] == w["ms_per_step_rank_max"] == w["ms_per_step_per_rank"][0] <= w["ms_per_step"]
    assert t["roofline"]["kernel"] == "k_merkle4" and s["roofline"]["kernel"] == "k_sponge_lines"
    cb = d["cpu_baseline"]
    assert cb["parity_samples"] == {"merkle4_digests": True, "tree": True, "forest": True, "sponge42": True, "openings": True, "encrypt": True, "extract": True} and cb["parity_sample_ok"] is True
    # `cores` = the CPUs the box grants (quota / affinity), `threads` = what the fastest run started; the reference's cargo bench is
    # probed at run time (no Rust toolchain on these boxes: reported unavailable with what was missing, never assumed)
    assert cb["threads"] >= 1 and 1 <= cb["cores"] <= cb["cpus_visible"] and "cpu_quota" in cb
    assert cb["value_per_quota_cpu"] == pytest.approx(cb["value"] / cb["cores"])
    rc = cb["reference_cargo_bench"]
    assert rc["available"] in (True, False) and set(rc["probe"]) == {"cargo", "rustc", "reference_dir", "crate_registry"}
    assert rc["available"] or rc["why"]


@pytest.mark.parametrize("workload,log2n,kernel", [("sponge42", "14", "k_sponge_lines"), ("openings", "14", "k_merkle4_path_lines"), ("tree", "14", "k_merkle4"), ("forest", "16", "k_merkle4"), ("extract", "12", "k_merkle4_openings"),
                                                   ("encrypt", "14", "k_crypt"),
                                                   # batches of <= 8,192 items run (and are priced as) the lane-group kernels
                                                   ("sponge42", "12", "k_sponge_coop"), ("openings", "11", "k_merkle4_path_coop"),
                                                   ("encrypt", "12", "k_crypt_coop"), ("merkle4_digests", "12", "k_merkle4_coop<8>"),
                                                   ("merkle4_digests", "14", "k_merkle4_coop<4>")])
def test_bench_other_workloads(gpu_ctx, workload, log2n, kernel):
    """the non-default workloads (configs[2], configs[3], the openings of SURVEY §8 f3): same contract, self-consistency
    (the oracle check of a sample of what each of them times runs once, in test_bench_default_line_carries_the_secondary_workloads)"""
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--workload", workload,
                                   "--log2n", log2n, "--no-cpu-baseline"], cwd=ROOT, timeout=900, stderr=subprocess.DEVNULL)
    d = _one_json_line(out)
    assert d["self_consistency_ok"] is True
    assert d["roofline"]["kernel"] == kernel and d["value"] > 1e5


def test_bench_rccl_backend_single_rank(gpu_ctx):
    """the real nccl (= RCCL) process group on the GPU: init, table broadcast, barrier, all-reduce —
    one rank is all a 1-GPU box allows, but it is the same code path the 8-GPU run takes"""
    env = dict(os.environ, P252_BENCH_FORCE_DIST="1", MASTER_PORT=str(_free_port()))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
                                   "--log2n", "14", "--secondary-log2n", "12", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, timeout=600,
                                  stderr=subprocess.DEVNULL)
    line, d = _one_json_line(out, want_detail=True)
    assert d["n_gpus"] == 1 and d["self_consistency_ok"] is True and line["config"]["constants_identical_on_all_ranks"] is True
    assert "inside libposeidon252_hip.so" in line["secondary"]["tree"]["exchange_impl"]
    assert "identical to local derivation: True" in d["config"]["constants"]
    # the secondary tree takes the sharded path whenever a process group exists: subtree root -> RCCL all-gather (of one
    # root here) -> top levels — the collective of BASELINE configs[4] on the real backend, INSIDE the library (VERDICT r3
    # item 3): ncclCommInitRank with the id handed round by torch.distributed, the constants broadcast and validated at
    # creation, ncclAllGather on the launch stream
    t = d["secondary"]["tree"]
    assert "inside libposeidon252_hip.so" in t["exchange_impl"], t["exchange_impl"]
    assert t["collective_backend"] == "nccl" and "all-gather of 1 x 32-byte subtree roots" in t["exchange"] and t["self_consistency_ok"] is True
    assert t["units_per_gpu_per_step"] == (4 ** 8 - 1) // 3 and d["secondary"]["sponge42"]["self_consistency_ok"] is True


def test_n1_value_is_the_same_with_and_without_a_process_group(gpu_ctx):
    """the driver's SCALE curve starts with an N = 1 point that may be launched through torch.distributed.run; it must
    agree with BENCH's plain `python bench.py`.  The primary (configs[1], 2^20 digests per step, default steps / warmup) timed twice on
    this box — plain, and with a one-rank RCCL process group (barrier + max-over-ranks around the timed region) — within 2 %
    (measured: 0.1-0.4 %, profiles/r06_n1_dist_vs_plain.txt)."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-secondary", "--no-cpu-baseline", "--no-check"]
    vals = {}
    for name, extra in (("plain", {}), ("dist", {"P252_BENCH_FORCE_DIST": "1", "MASTER_PORT": str(_free_port())})):
        env = dict(os.environ, **extra)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out = subprocess.check_output(base, cwd=ROOT, env=env, timeout=600, stderr=subprocess.DEVNULL)
        line = _one_json_line(out)
        assert line["n_gpus"] == 1 and line["config"]["units_per_gpu_per_step"] == 1 << 20
        vals[name] = line["value"]
    ratio = vals["dist"] / vals["plain"]
    print("N=1 primary: plain %.4g, with a process group %.4g, ratio %.4f" % (vals["plain"], vals["dist"], ratio))
    assert 0.98 < ratio < 1.02, vals


def test_bench_tree_two_ranks_gather_roots(gpu_ctx):
    """configs[4] structure at small scale: per-rank subtree, all-gather of the roots, top levels"""
    env = dict(os.environ, P252_BENCH_SHARE_GPU="1", P252_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--workload", "tree", "--log2n", "12"]
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, timeout=900, stderr=subprocess.DEVNULL)
    d = _one_json_line(out)
    assert d["n_gpus"] == 2 and d["self_consistency_ok"] is True
    assert "all-gather of 2 subtree roots" in d["config"]["workload"]
    assert d["config"]["units_per_gpu_per_step"] == 1365 + 1  # 4^6 leaves -> 1365 nodes, + 1 top node over 2 roots


def test_bench_two_ranks_share_gpu_gloo(gpu_ctx):
    env = dict(os.environ, P252_BENCH_SHARE_GPU="1", P252_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--log2n", "16", "--secondary-log2n", "12", "--full"]
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, timeout=900, stderr=subprocess.DEVNULL)
    line, d = _one_json_line(out, want_detail=True)
    assert line["n_gpus"] == 2 and line["config"]["ranks"] == 2 and line["value"] == pytest.approx(2 * line["config"]["units_per_gpu_per_step"] * 3 / (line["ms_per_step"] * 3e-3), rel=1e-6)
    assert d["n_gpus"] == 2 and d["self_consistency_ok"] is True and "cpu_baseline" not in d
    assert "identical to local derivation: True" in d["config"]["constants"]
    # whole-job value = 2 ranks x units / max-over-ranks time
    assert d["value"] == pytest.approx(2 * d["config"]["units_per_gpu_per_step"] * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)
    # the secondary workloads at N = 2: the tree is the configs[4] composition (subtree per rank, all-gather of the roots)
    t, s = d["secondary"]["tree"], d["secondary"]["sponge42"]
    assert t["n_gpus"] == 2 and t["ranks"] == 2 and t["collective_backend"] == "gloo" and "all-gather of 2 x 32-byte subtree roots" in t["exchange"]
    assert "all-gather of 2 subtree roots" in t["workload"] and t["units_per_gpu_per_step"] == (4 ** 8 - 1) // 3 + 1
    # whole-job units: both subtrees + the one top node once (every rank hashes it; it is not counted twice)
    assert t["units_whole_job_per_step"] == 2 * ((4 ** 8 - 1) // 3) + 1
    assert t["value"] == pytest.approx(t["units_whole_job_per_step"] * t["steps"] / (t["ms_per_step"] * t["steps"] * 1e-3), rel=1e-6)
    assert "torch.distributed" in t["exchange_impl"] and "gloo" in t["exchange_impl"]  # (ranks sharing a GPU: RCCL wants a device per rank)
    assert len(t["ms_per_step_per_rank"]) == 2 and t["ms_per_step_rank_min"] <= t["ms_per_step_rank_max"] <= t["ms_per_step"] * 1.001
    assert s["ranks"] == 2 and s["exchange"] is None and s["units_per_gpu_per_step"] == 12 << 12
    for w in (t, s):
        assert w["self_consistency_ok"] is True and w["parity_sample_ok"] is None  # (the oracle leg exists at N = 1 only)
        assert w["roofline"]["clock"]["ghz_measured"] > 1.0


def _rehearse_the_driver_command(oracle_mod, world, share_gpu):
    """`python bench.py --gpus <world> --steps K --warmup W --full` at scaled-down sizes: rendezvous, the world-way configs[4] composition of
    the secondary tree (world subtrees, all-gather of world x 32-byte roots, zero-padded top levels), the whole-job unit count,
    per-rank times — and the root equals the oracle's tree over the CONCATENATION of the ranks' leaves"""
    import numpy as np
    import poseidon252_amd as P
    k = 6  # 4^6 leaves per rank
    env = dict(os.environ, MASTER_PORT=str(_free_port()))
    if share_gpu:
        env.update(P252_BENCH_SHARE_GPU="1", P252_BENCH_BACKEND="gloo")
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR"):
        env.pop(key, None)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1",
                                   "--log2n", "12", "--secondary-log2n", str(2 * k - 4), "--full"], cwd=ROOT, env=env, timeout=1500, stderr=subprocess.DEVNULL)
    line, d = _one_json_line(out, want_detail=True)  # the multi-rank line (per-rank arrays live in the side file) stays inside the budget too
    top = P.levels_len(world)
    assert line["n_gpus"] == world and line["config"]["ranks"] == world and line["ms_per_step_rank_min"] <= line["ms_per_step_rank_max"]
    assert line["secondary"]["tree"]["units_whole_job_per_step"] == world * ((4 ** k - 1) // 3) + top
    assert d["n_gpus"] == world and d["config"]["ranks"] == world and d["self_consistency_ok"] is True and "cpu_baseline" not in d
    assert d["value"] == pytest.approx(world * d["config"]["units_per_gpu_per_step"] * 2 / (d["ms_per_step"] * 2e-3), rel=1e-6)
    assert len(d["ms_per_step_per_rank"]) == world and d["ms_per_step_rank_min"] <= d["ms_per_step_rank_max"] <= d["ms_per_step"] * 1.001
    t = d["secondary"]["tree"]
    assert "all-gather of %d subtree roots" % world in t["workload"]
    if world == 8:
        assert "BASELINE configs[4]" in t["workload"] and "8 x 2^%d leaves" % (2 * k) in t["workload"]
    assert "all-gather of %d x 32-byte subtree roots" % world in t["exchange"] and t["ranks"] == world and t["n_gpus"] == world
    sub = (4 ** k - 1) // 3
    assert t["units_per_gpu_per_step"] == sub + top and t["units_whole_job_per_step"] == world * sub + top
    assert t["value"] == pytest.approx(t["units_whole_job_per_step"] * t["steps"] / (t["ms_per_step"] * t["steps"] * 1e-3), rel=1e-6)
    assert t["self_consistency_ok"] is True and len(t["ms_per_step_per_rank"]) == world
    # rank r's leaves are the SURVEY §8(d) stream of seed 0xc10d + r (bench.py make_workload; the device generator is
    # byte-identical to the oracle's fill_random, tests/test_synth.py)
    leaves = np.concatenate([oracle_mod.fill_random(0xC10D + r, 4 ** k) for r in range(world)])
    root = oracle_mod.merkle4_tree(P.merkle4_tag(), leaves)[0]
    assert t["root_mont_hex"] == "".join("%016x" % int(v) for v in root[::-1]), (t["root_mont_hex"], root)
    for w in d["secondary"].values():
        assert w["self_consistency_ok"] is True and w["ranks"] == world


def test_bench_eight_ranks_rehearsal_of_the_driver_command(gpu_ctx, oracle_mod):
    """the exact command the driver runs on the 8-GPU node — `python bench.py --gpus 8 --steps K --warmup W`, one
    rank per GPU — including the 8-way configs[4] composition (8 subtrees, top nodes [n0, n1, 0, 0] and their parent, hash.rs:22-26).
    Eight ranks sharing one GPU would hold it open in nine processes with this runner: on a box with fewer GPUs the library's 8-way
    composition is covered by tests/test_comm_mock_ranks.py (one thread per rank) and the command by the 3-rank rehearsal below."""
    import torch
    if torch.cuda.device_count() < 8:
        pytest.skip("needs 8 GPUs (one rank per GPU), found %d" % torch.cuda.device_count())
    _rehearse_the_driver_command(oracle_mod, 8, share_gpu=False)


def test_bench_three_ranks_share_gpu_rehearsal_of_the_driver_command(gpu_ctx, oracle_mod):
    """the driver's command shape with 3 ranks that share this box's one GPU (gloo collectives): an odd number of subtree roots, so the
    top level is zero-padded ([r0, r1, r2, 0]) as at 8 ranks; four processes hold the GPU (the runner and three ranks)"""
    _rehearse_the_driver_command(oracle_mod, 3, share_gpu=True)


def test_bench_watchdog_prints_the_line_when_a_secondary_hangs(gpu_ctx):
    """N > 1: a secondary workload that never returns (a collective hanging on a node this code has never seen) must cost that
    workload, not the run — the primary figures are what the scaling curve is made of.  Past --secondary-timeout rank 0 prints
    the line with what was measured and `secondary_timeout`, every rank exits 0."""
    env = dict(os.environ, P252_BENCH_SHARE_GPU="1", P252_BENCH_BACKEND="gloo", P252_BENCH_TEST_HANG="sponge42")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--log2n", "12", "--secondary-log2n", "8", "--secondary-timeout", "8", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=600, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d, full = _one_json_line(r.stdout, want_detail=True)  # (the watchdog prints the same bounded line)
    assert d["n_gpus"] == 2 and d["value"] > 1e5 and d["self_consistency_ok"] is True
    assert d["secondary_timeout"]["workload"] == "sponge42" and sorted(d["secondary"]) == ["forest", "tree"]
    assert d["secondary"]["tree"]["self_consistency_ok"] is True and full["secondary_timeout"]["workload"] == "sponge42"
    # the primary's minimal record went to stderr as soon as it was measured — a kill during a secondary
    # (which no watchdog sees) still leaves the scaling number in the captured tail
    prim = [l for l in r.stderr.decode().splitlines() if l.startswith("bench.py primary: ")]
    assert len(prim) == 1
    rec = json.loads(prim[0][len("bench.py primary: "):])
    assert rec["n_gpus"] == 2 and rec["value"] == pytest.approx(d["value"], rel=1e-6) and rec["ms_per_step"] == pytest.approx(d["ms_per_step"], rel=1e-6)
    assert rec["roofline_frac"] == pytest.approx(d["roofline"]["frac"], rel=1e-5)


def test_bench_gpus_flag_launches_the_ranks_itself(gpu_ctx):
    """`python bench.py --gpus 2` with NO launcher: bench.py re-executes itself under torch.distributed.run, so
    --gpus can never be silently ignored.  2 ranks share the one GPU here (test-only switches)."""
    env = dict(os.environ, P252_BENCH_SHARE_GPU="1", P252_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                                   "--log2n", "14"], cwd=ROOT, env=env, timeout=900, stderr=subprocess.DEVNULL)
    d = _one_json_line(out)
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["config"]["collective_backend"] == "gloo"
    assert d["self_consistency_ok"] is True


def test_bench_refuses_more_ranks_than_devices(gpu_ctx):
    """one rank per GPU: asking for 2 GPUs on a 1-GPU box is an error, not a 1-GPU number"""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with a single GPU")
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "P252_BENCH_SHARE_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--log2n", "12",
                        "--no-cpu-baseline"], cwd=ROOT, env=env, timeout=600, capture_output=True)
    assert r.returncode != 0
    assert not [l for l in r.stdout.decode().splitlines() if l.strip().startswith("{")]


def test_bench_plain_run_times_the_primary_alone_and_dumps_what_full_dumps(gpu_ctx, tmp_path):
    """a plain run (no --full) times and self-checks the primary and nothing else: no secondary workload, no cpu_baseline leg.  With
    --dump-outputs it times the secondaries too, whose outputs the files hold, and writes what a --full run of the same command line
    writes, file for file (the default primary, 2^20 digests, is a sample of rows in half the budget)"""
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--secondary-log2n", "8"]
    runs = {}
    for name, extra in (("plain", []), ("plain_dump", ["--dump-outputs", str(tmp_path / "plain_dump")]),
                        ("full_dump", ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full_dump")])):
        r = subprocess.run(base + extra, cwd=ROOT, timeout=900, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        runs[name] = (_one_json_line(r.stdout), r.stderr.decode())
    line, err = runs["plain"]
    assert "secondary" not in line and "cpu_baseline" not in line and line["self_consistency_ok"] is True
    assert line["steps"] == 2 and line["config"]["units_per_gpu_per_step"] == 1 << 20 and "bench.py: secondary" not in err
    secondaries = ["encrypt", "extract", "forest", "openings", "sponge42", "tree"]
    for name in ("plain_dump", "full_dump"):
        assert sorted(runs[name][0]["secondary"]) == secondaries and "cpu_baseline" not in runs[name][0]
    files = sorted(os.listdir(str(tmp_path / "plain_dump")))
    assert files == sorted(os.listdir(str(tmp_path / "full_dump")))
    assert set(k + "_rows.npy" for k in ["merkle4_digests"] + secondaries) <= set(files)
    assert 0 < len(np.load(str(tmp_path / "plain_dump" / "merkle4_digests_rows.npy"))) < (1 << 20)
    for f in files:
        assert np.array_equal(np.load(str(tmp_path / "plain_dump" / f)), np.load(str(tmp_path / "full_dump" / f))), f


def test_bench_dump_outputs_are_what_the_timed_steps_computed(gpu_ctx, oracle_mod, tmp_path):
    """--dump-outputs DIR: every timed workload's outputs as float64 .npy (64-bit words as exact 32-bit halves), inside 64 MB; the
    primary's digests, the tree's root and the sponges are the oracle's on the same seeded inputs; --steps sets the timed steps"""
    import numpy as np
    import poseidon252_amd as P
    d_dir = tmp_path / "out"
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--log2n", "12",
                                   "--secondary-log2n", "8", "--no-cpu-baseline", "--dump-outputs", str(d_dir)], cwd=ROOT, timeout=900,
                                  stderr=subprocess.DEVNULL)
    line = _one_json_line(out)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    files = {f: np.load(str(d_dir / f)) for f in os.listdir(str(d_dir))}
    assert all(a.dtype == np.float64 for a in files.values()) and sum(os.path.getsize(str(d_dir / f)) for f in files) <= 64 << 20
    for key in ("merkle4_digests", "tree", "forest", "sponge42", "openings", "encrypt", "extract"):
        assert key + "_rows.npy" in files, sorted(files)
    words = lambda a: (a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32)))
    n = 1 << 12
    assert np.array_equal(files["merkle4_digests_rows.npy"], np.arange(n))
    x = oracle_mod.fill_random(0xC10D, 4 * n).reshape(n, 4, 4)
    assert np.array_equal(words(files["merkle4_digests_digests.npy"]), oracle_mod.hash_batch(P.merkle4_tag(), x, 4, 1, threads=8).reshape(n, 4))
    root = oracle_mod.merkle4_tree(P.merkle4_tag(), oracle_mod.fill_random(0xC10D, 1 << 12))[0]
    assert np.array_equal(words(files["tree_root.npy"]).reshape(4), root)
    rows = files["sponge42_rows.npy"].astype(np.int64)
    m = oracle_mod.fill_random(0xC10D, 42 << 8).reshape(1 << 8, 42, 4)[rows]
    tag = P.HashBatch(P.Domain.Other, 42, output_len=5, ctx=gpu_ctx).tag
    assert np.array_equal(words(files["sponge42_outputs.npy"]).reshape(-1), oracle_mod.hash_batch(tag, m, 42, 5).reshape(-1))
    assert files["extract_out_of_range.npy"].tolist() == [0.0]
