"""bench.py's roofline arithmetic without a GPU: the top-level scalars of `roofline` are the HARDWARE fraction —
executed multiply-adds (ISA-derived count from profiles/) x units per launch / launch time / (1024 SIMDs x 2.4 GHz / 4 x 64 lanes) —
with SURVEY §8d's 256,000-MAC reference-schedule pricing under its own name; the HBM-shaped roofline of the extraction workload;
counter traffic from the committed passes.  The numbers fed in are round 4's measured launch times, so the expected fractions are
the ones DESIGN.md quotes."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _w(key, n, units, **kw):
    W = types.SimpleNamespace(key=key, n=n, perms_per_step=units, **kw)
    return W


CLK = {"shader_ghz": 2.36, "interval_us": 3000.0, "cycles_per_dependent_add": 44.0}


def test_digest_roofline_is_the_hardware_fraction():
    W = _w("merkle4_digests", 1 << 20, 1 << 20)
    r = bench.roofline_of(W, [2.108, 2.110, 2.106], CLK, dict(CLK, shader_ghz=2.362))
    assert r["bound"] == "valu-int32-mac" and r["kernel"] == "k_merkle4" and r["unit"] == "TMAC/s"
    assert r["peak"] == pytest.approx(1024 * 2.4e9 / 4 * 64 / 1e12) == pytest.approx(39.3216)
    assert r["macs_per_perm_executed"] == 61237 and r["valu_insts_per_perm"] == 76983  # profiles/r03_isa_counts.json (kernels unchanged since)
    assert r["achieved"] == pytest.approx(61237 * (1 << 20) / 2.108e-3 / 1e12, rel=1e-3)
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"]) and 0.77 < r["frac"] < 0.78
    assert r["clock_ghz_measured"] == pytest.approx(2.361) and r["frac_at_measured_clock"] == pytest.approx(r["frac"] * 2.4 / 2.361)
    assert r["frac"] < r["frac_valu_issue"] < 1 and r["frac_valu_issue"] == pytest.approx(288104 / 4 / 61237 * r["frac"], rel=1e-6)
    # the reference schedule's pricing is kept, under its own name, and is NOT the fraction
    assert r["frac_reference_schedule"] == pytest.approx(r["frac"] * 256000 / 61237) and r["frac_reference_schedule"] > 3
    assert r["achieved_reference_schedule"] == pytest.approx(256000 * (1 << 20) / (r["launch_ms_mean"] * 1e-3) / 1e12)
    # counter traffic of the committed pass, per launch, next to the algorithmic bytes
    assert r["traffic_algorithmic_bytes"] == 160.0 * (1 << 20)
    # (1.009 on three boxes of rounds 3-5, 1.016 on the box of round 5's final set: a few hundred KB of instruction and constant fetches)
    assert 1.005 < r["traffic_ratio"] < 1.02 and r["traffic"] == pytest.approx(r["traffic_ratio"] * 160 * (1 << 20), rel=1e-9)
    assert r["hbm_frac"] < 0.011
    for k, v in r.items():  # what the driver's record keeps: every headline figure is a top-level scalar
        if k in ("achieved", "peak", "frac", "frac_at_measured_clock", "frac_valu_issue", "macs_per_perm_executed", "clock_ghz_measured", "traffic",
                 "traffic_ratio", "frac_reference_schedule", "launch_ms_mean"):
            assert isinstance(v, (int, float)) and not isinstance(v, bool), k


def test_small_batches_are_priced_as_the_lane_group_kernels():
    r = bench.roofline_of(_w("merkle4_digests", 4096, 4096), [0.115], CLK, CLK)
    assert r["kernel"] == "k_merkle4_coop<8>" and r["macs_per_perm_executed"] == 8 * r["executed"]["macs_per_perm"] // 8
    # eight lanes per digest: 32,768 lanes = one wave on half of the SIMDs, each lane issuing 37.8 k multiply-adds in 0.115 ms
    assert r["valu_issue"]["lanes_per_perm"] == 8 and 0.2 < r["frac"] < 0.35
    r4 = bench.roofline_of(_w("merkle4_digests", 16384, 16384), [0.128], CLK, CLK)
    assert r4["kernel"] == "k_merkle4_coop<4>" and r4["valu_issue"]["lanes_per_perm"] == 4


def test_tree_and_forest_traffic_come_from_the_tree_passes():
    units = (4 ** 12 - 1) // 3
    t = bench.roofline_of(_w("tree", 1 << 24, units), [12.2], CLK, CLK)
    assert t["kernel"] == "k_merkle4" and t["traffic_ratio"] == pytest.approx(1.714, rel=2e-3)
    assert t["traffic_detail"]["ratio_level_by_level"] == pytest.approx(1.03, abs=0.01)  # against what a level-by-level build must move
    bench.BYTES_PER_PERM["forest"] = (4096 * 32 + 32) / 1365.0
    f = bench.roofline_of(_w("forest", 1 << 24, 4096 * 1365), [11.66], CLK, CLK)
    assert f["kernel"] == "k_merkle4" and f["frac"] > t["frac"] and f["traffic_ratio"] == pytest.approx(1.713, rel=3e-3)


def test_extraction_is_priced_against_the_hbm_roofline_from_the_r07_passes():
    k, depth = 1 << 20, 12
    W = _w("extract", k, k * depth, bytes_per_unit=96.0 + 96.0 + 1.0 + 68.0 / depth)
    r = bench.roofline_of(W, [0.616, 0.614], CLK, CLK)
    assert r["bound"] == "hbm" and r["kernel"] == "k_merkle4_openings" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    alg = k * (depth * 193 + 68)
    assert r["traffic_algorithmic_bytes"] == pytest.approx(alg) and r["achieved"] == pytest.approx(alg / 0.615e-3 / 1e9, rel=1e-6)
    assert r["frac"] == pytest.approx(r["achieved"] / 8000.0) and 0.50 < r["frac"] < 0.52
    # round 5's FAST build (0.580 ms, profiles/r05_openings_extract.txt): 0.54 — the ceiling of this access pattern (k_gather16 on the same box)
    assert 0.53 < bench.roofline_of(W, [0.580], CLK, CLK)["frac"] < 0.55
    # the committed FETCH x 2 + WRITE passes of the final kernel (scratch 0; round 6's exact-division build, re-collected in round 7 for the
    # shared kernel sources: 74 VALU instructions per wave as before): reads below algorithmic (upper levels hit in cache), writes equal
    assert r["traffic_source"] == "profiles/r07_pmc_k_merkle4_openings.json" and r["traffic_ratio"] == pytest.approx(0.823, abs=0.005)


def test_cpu_baseline_plumbing_probes_at_run_time():
    rc = bench.reference_cargo_bench()
    assert set(rc["probe"]) == {"cargo", "rustc", "reference_dir", "crate_registry"} and rc["command"].startswith("cargo bench --features=zk --bench hash")
    if not rc["available"]:
        assert rc["why"].startswith("not on this box: ") and all(name in rc["why"] for name, v in rc["probe"].items() if not v)
    assert 1 <= bench.usable_cpus() <= (os.cpu_count() or 1)


def _full_record():
    """round 4's real 26 KB record (all six secondaries, cpu_baseline): the one the driver could NOT parse"""
    import json
    return json.load(open(os.path.join(ROOT, "profiles", "r04_bench.json")))


def test_printed_line_fits_the_drivers_tail_and_is_scalars_only(tmp_path, capsys):
    """BENCH_r04.json had parsed = null because the line was 26,409 bytes against the driver's 8 KB tail.  The
    printed line is now scalars only, under 6,000 bytes with all six secondaries and the cpu_baseline; the full record goes to a side file."""
    import json
    full = _full_record()
    assert len(json.dumps(full)) > 20000
    line = bench.emit(full, str(tmp_path / "bench_detail.json"))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and len(out) < bench.LINE_BUDGET_BYTES == 6000 and json.loads(out) == line and "line_trimmed" not in line
    assert json.load(open(tmp_path / "bench_detail.json")) == full  # nothing is lost: every nested model, source and note is in the side file
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert line[k] == (pytest.approx(full[k], rel=1e-8) if isinstance(full[k], float) else full[k]), k
    assert line["config"]["workload"] == full["config"]["workload"] and line["config"]["units_per_gpu_per_step"] == 1 << 20
    r = line["roofline"]
    assert set(r) == set(bench.ROOFLINE_SCALARS) and all(v is None or isinstance(v, (int, float, str)) for v in r.values())
    assert r["bound"] == "valu-int32-mac" and r["kernel"] == "k_merkle4" and r["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-6)
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-5) and r["traffic"] == pytest.approx(full["roofline"]["traffic"], rel=1e-6)
    assert sorted(line["secondary"]) == ["encrypt", "extract", "forest", "openings", "sponge42", "tree"]
    for key, w in line["secondary"].items():
        assert all(v is None or isinstance(v, (bool, int, float, str)) for v in w.values()), key
        assert w["value"] == pytest.approx(full["secondary"][key]["value"], rel=1e-8) and w["frac"] == pytest.approx(full["secondary"][key]["roofline"]["frac"], rel=1e-6)
        assert w["kernel"] == full["secondary"][key]["roofline"]["kernel"] and w["self_consistency_ok"] is True and w["parity_sample_ok"] is True
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 16 and cb["value"] == pytest.approx(full["cpu_baseline"]["value"], rel=1e-6) and cb["sample"]
    assert cb["reference_cargo_bench"] == {"available": False, "value": None} and cb["parity_sample_ok"] is True


def test_eight_rank_line_with_long_strings_stays_inside_the_budget(tmp_path, capsys):
    """the N = 8 line: per-rank arrays and the exchange descriptions must not push it past the budget either (they live in the side file)"""
    import copy
    import json
    full = copy.deepcopy(_full_record())
    full.pop("cpu_baseline")
    full["n_gpus"] = 8
    full["ms_per_step_per_rank"] = [2.123456789012] * 8
    full["config"].update(ranks=8, collective_backend="nccl", units_whole_job_per_step=8 << 20)
    for w in full["secondary"].values():
        w["ms_per_step_per_rank"] = [12.123456789012] * 8
        w["exchange_impl"] = "ncclAllGather inside libposeidon252_hip.so (p252_merkle4_tree_sharded_device), on the launch stream; " + "x" * 300
        w["workload"] += " = 2^27-leaf tree sharded across 8 GPUs (BASELINE configs[4])" + " padding" * 40
        w["root_mont_hex"] = "f" * 64
    full["secondary_timeout"] = {"workload": "extract", "seconds": 240, "note": "n" * 500}
    line = bench.emit(full, str(tmp_path / "d.json"))
    out = capsys.readouterr().out
    assert len(out) < bench.LINE_BUDGET_BYTES and "line_trimmed" not in line and line["secondary_timeout"] == {"workload": "extract", "seconds": 240}
    assert "ms_per_step_per_rank" not in json.dumps(line) and line["n_gpus"] == 8 and line["config"]["ranks"] == 8


def test_primary_record_goes_to_stderr_at_once(capsys):
    """a minimal primary record on stderr as soon as the primary is measured"""
    import json
    bench.primary_record_to_stderr(_full_record())
    err = capsys.readouterr().err
    assert err.startswith("bench.py primary: ") and len(err) < 400
    rec = json.loads(err[len("bench.py primary: "):])
    assert rec["value"] == pytest.approx(4.945e8, rel=1e-3) and rec["roofline_frac"] == pytest.approx(0.7705, rel=1e-3) and rec["n_gpus"] == 1


def test_stdout_carries_exactly_one_line_whatever_libraries_print(tmp_path):
    """RCCL prints its version banner to fd 1 when a communicator is created (seen in the GPU suite's log): bench.py points fd 1 at
    stderr for the run and writes the line to the real stdout — a driver reading stdout sees ONE line, the JSON"""
    import json
    import subprocess
    code = ("import os, sys, json; sys.path.insert(0, %r); import bench\n"
            "bench.keep_stdout_for_the_line()\n"
            "os.write(1, b'RCCL version : 2.26.6-HEAD:64f48b6\\nHIP version  : 7.0\\n')\n"  # a C library writing to fd 1
            "print('a python print as well')\n"
            "bench.emit(json.load(open(%r)), %r)\n" % (ROOT, os.path.join(ROOT, "profiles", "r04_bench.json"), str(tmp_path / "d.json")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["metric"].startswith("Poseidon width-5") and len(lines[0]) < 6000
    assert b"RCCL version" in r.stderr and b"a python print as well" in r.stderr
