"""bench.py --dump-outputs without a GPU: the host side of the snapshot (exact float64 image of the 64-bit limbs, the byte budget,
the fixed seeded row sample shared by every per-item array) on CPU tensors standing in for the device arrays."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _limbs(a):
    """the uint64 words back from the (low, high) float64 halves"""
    return a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32))


def test_exact_float64_keeps_every_bit():
    w = np.array([0, 1, 0xFFFFFFFF, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001], dtype=np.uint64)
    f = bench._exact_float64(w.view(np.int64))
    assert f.dtype == np.float64 and f.shape == (6, 2)
    assert np.array_equal(_limbs(f), w)
    assert np.array_equal(bench._exact_float64(np.array([3, 250], dtype=np.uint8)), [3.0, 250.0])


def test_snapshot_takes_every_row_when_it_fits(tmp_path):
    d = torch.arange(64 * 4, dtype=torch.int64).view(64, 4) * -7
    W = types.SimpleNamespace(outputs=[("digests", d)])
    snap = bench.snapshot_outputs(W, 1 << 20)
    assert sorted(snap) == ["digests", "rows"] and np.array_equal(snap["rows"], np.arange(64))
    assert np.array_equal(_limbs(snap["digests"]), d.numpy().view(np.uint64))
    bench.write_outputs(str(tmp_path / "out"), "merkle4_digests", snap)
    back = np.load(str(tmp_path / "out" / "merkle4_digests_digests.npy"))
    assert back.dtype == np.float64 and np.array_equal(back, snap["digests"])


def test_snapshot_samples_the_same_rows_of_every_array_within_the_budget():
    n, depth = 5000, 6
    g = torch.Generator().manual_seed(3)
    leaves = torch.randint(-(1 << 62), 1 << 62, (n, 4), dtype=torch.int64, generator=g)
    sib = torch.randint(-(1 << 62), 1 << 62, (n, depth, 3, 4), dtype=torch.int64, generator=g)
    pos = torch.randint(0, 4, (n, depth), dtype=torch.uint8, generator=g)
    bad = torch.zeros(1, dtype=torch.int32)
    W = types.SimpleNamespace(outputs=[("leaves", leaves), ("siblings", sib), ("positions", pos), ("out_of_range", bad)])
    budget = 200_000
    snap = bench.snapshot_outputs(W, budget)
    rows = snap["rows"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert sum(a.nbytes + 128 for a in snap.values()) <= budget
    assert np.array_equal(_limbs(snap["leaves"]), leaves.numpy()[rows].view(np.uint64))
    assert np.array_equal(_limbs(snap["siblings"]), sib.numpy()[rows].view(np.uint64))
    assert np.array_equal(snap["positions"], pos.numpy()[rows]) and np.array_equal(snap["out_of_range"], [0.0])
    # the sample is fixed: the same arguments give the same rows
    assert np.array_equal(bench.snapshot_outputs(W, budget)["rows"], snap["rows"])


def test_default_primary_dump_fits_the_budget():
    """the default primary (2^20 digests) shares the 64 MB with six secondaries: its half is a sample, inside the budget"""
    W = types.SimpleNamespace(outputs=[("digests", torch.zeros((1 << 20, 4), dtype=torch.int64))])
    snap = bench.snapshot_outputs(W, bench.DUMP_BUDGET_BYTES // 2)
    assert sum(a.nbytes + 128 for a in snap.values()) <= bench.DUMP_BUDGET_BYTES // 2 and len(snap["rows"]) > (1 << 18)
