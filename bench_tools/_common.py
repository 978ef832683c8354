"""What the Python bench tools share: the import path (the repository root, for the package and for testsupport: the tree geometry and
the numpy models), the shader-clock probe, the host-to-device copy, the timers and the set-ups two tools use alike.  A tool measures;
the models it compares counts with live in testsupport/, and no tool imports another tool."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from testsupport.treeshape import levels_bound, offsets  # noqa: E402


def clock_mhz(ctx):
    """shader clock of one probe wave (MHz), or None"""
    import torch
    try:
        t = ctx.clock_probe(spin_us=1000)
        torch.cuda.synchronize()
        return round(ctx.clock_probe_result(t)["shader_ghz"] * 1e3, 1)
    except Exception:  # (a measurement aid only)
        return None


def dev(a):
    """a numpy array on the device; uint64 / uint32 as the int64 / int32 torch has"""
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(a).to("cuda:0")


def once_ms(fn):
    """the host clock around one call that ends in a device synchronise"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    """one launch of fn between two device events on the current stream"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps, timer=once_ms):
    return float(np.median([timer(fn) for _ in range(reps)]))


def alternate(fns, reps, timer):
    """medians (ms) of the callables, run in turn `reps` times"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(timer(fn))
    return [float(np.median(t)) for t in ts]


class Forest:
    """a built forest (tree-major levels) on the device: the update and the journal tools' set-up"""

    def __init__(self, ctx, arity, sizes, max_leaves):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.arity, self.sizes, self.n_trees, self.max_leaves = ctx, arity, np.asarray(sizes, dtype=np.int64), len(sizes), max_leaves
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        self.off = offsets(sizes)
        n_leaves = int(self.off[-1])
        device = torch.device("cuda:0")
        self.d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device=device)
        self.d_off = dev(self.off)
        self.roots = torch.empty((self.n_trees, 4), dtype=torch.int64, device=device)
        self.d_lv = torch.empty((levels_bound(n_leaves, self.n_trees, max_leaves, arity) + 1, 4), dtype=torch.int64, device=device)
        self.build()

    def build(self):
        self.ctx.merkle_forest_ragged_device(self.tag, self.d, self.d_off, self.n_trees, self.max_leaves, self.roots, self.d_lv, arity=self.arity)


class Case:
    """an old forest built on the device, an append to it, and the buffers of the appended and of the freshly built new forest: the append
    and the resize tools' set-up"""

    def __init__(self, ctx, arity, sizes, adds):
        import torch
        from poseidon252_amd import merkle as M
        self.ctx, self.arity = ctx, arity
        sizes, adds = np.asarray(sizes, dtype=np.int64), np.asarray(adds, dtype=np.int64)
        self.T, self.n_leaves, self.n_add = len(sizes), int(sizes.sum()), int(adds.sum())
        self.max_old, self.max_new = int(sizes.max()), int((sizes + adds).max())
        self.tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
        device = torch.device("cuda:0")
        self.d_off, self.d_aoff = dev(offsets(sizes, dtype=np.int64)), dev(offsets(adds, dtype=np.int64))
        self.d = torch.randint(0, 1 << 60, (self.n_leaves, 4), dtype=torch.int64, device=device)
        self.d_add = torch.randint(0, 1 << 60, (self.n_add, 4), dtype=torch.int64, device=device) if self.n_add else None
        cap = lambda n, mx: levels_bound(n, self.T, mx, arity)  # noqa: E731
        self.lv = torch.empty((cap(self.n_leaves, self.max_old), 4), dtype=torch.int64, device=device)
        self.roots_old = torch.empty((self.T, 4), dtype=torch.int64, device=device)
        ctx.merkle_forest_ragged_device(self.tag, self.d, self.d_off, self.T, self.max_old, self.roots_old, self.lv, arity=arity)
        total = self.n_leaves + self.n_add
        new = lambda: (torch.zeros((total, 4), dtype=torch.int64, device=device), torch.zeros((cap(total, self.max_new), 4), dtype=torch.int64, device=device),  # noqa: E731
                       torch.zeros((self.T, 4), dtype=torch.int64, device=device))
        self.a_leaves, self.a_lv, self.a_roots = new()
        self.b_leaves, self.b_lv, self.b_roots = new()
        self.a_off = torch.zeros(self.T + 1, dtype=torch.int64, device=device)
        self.hashed = torch.zeros(1, dtype=torch.int64, device=device)
        self.bytes_moved = None

    def append(self, count=False):
        self.ctx.merkle_forest_ragged_append_device(self.tag, self.d, self.d_off, self.T, self.max_old, self.lv, self.d_add, self.d_aoff, self.T,
                                                    self.max_new, self.a_leaves, self.a_off, self.a_lv, self.a_roots, None,
                                                    self.hashed if count else None, arity=self.arity)

    def rebuild(self):
        """the fresh build of the new forest, from the append's own leaves and offsets"""
        self.ctx.merkle_forest_ragged_device(self.tag, self.a_leaves, self.a_off, self.T, self.max_new, self.b_roots, self.b_lv, arity=self.arity)

    def identical(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.equal(self.a_roots, self.b_roots)) and bool(torch.equal(self.a_lv, self.b_lv))
