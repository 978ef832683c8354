#!/usr/bin/env python3
"""Calls the ten ragged-forest entry points once each per shape, for a kernel trace: p252_merkle{4,2}_forest_ragged_device with and
without d_levels, ..._forest_ragged_openings_device, ..._path_ragged_device, ..._forest_ragged_verify_device and
..._forest_ragged_update_device, on a small forest (every level on the 8-lane-group digests) and a large one (the low levels on
the one-lane digests, the narrow top levels on the groups), with few and with many updates.  Then the calls that change or prove a
built forest, on the same two forests (the large one has more trees than one scan tile of 2,048, and its pairs fill more than one
256-element tile of the shared proof's list scan): ..._forest_ragged_update_journaled_device_into, ..._journal_swap_device_into (undo,
redo), ..._forest_ragged_multiproof_device and its _verify_, ..._forest_ragged_append_device_into and ..._resize_device_into.  Then the
other calls that work in the context's per-stream scratch, at one small and one chip-filling shape each: p252_hash_ragged_device,
root-only p252_merkle{4,2}_tree_device and p252_merkle{4,2}_forest_device, p252_merkle{4,2}_verify_batch_device and
p252_merkle{4,2}_multiproof[_verify]_device.

  rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python bench_tools/forest_dispatch_driver.py
  python bench_tools/forest_dispatch_driver.py --dispatches DIR/.../NAME_kernel_trace.csv     # the ordered dispatch list

Two builds of the library launch the same kernels in the same order with the same grids exactly when the lists are equal
(P252_LIB_PATH selects the library; P252_RAGGED_SORT=0, read once per process, the unsorted re-hash).  Every verify call must
accept every opening and every shared proof, before and after the updates, and every changed forest must have the roots of a fresh
build of its leaves: the driver exits non-zero otherwise."""
import argparse
import csv
import re
import sys

import numpy as np

import _common as C
from testsupport import treeshape as TS


def dispatches(path):
    """the trace's (kernel base name, grid, workgroup) rows in dispatch order, one per line"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        base = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Kernel_Name"])).replace("p252::", "").replace(".kd", "")
        print(base, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])


def run(ctx, arity, sizes, ks, seed):
    import torch
    from poseidon252_amd import merkle as M
    rng = np.random.default_rng(seed)
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    sizes = np.asarray(sizes, np.int64)
    n_trees, max_leaves = len(sizes), int(sizes.max())
    off = TS.offsets(sizes)
    n_leaves, D = int(off[-1]), TS.depth(max_leaves, arity)
    dev = torch.device("cuda:0")
    d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device=dev)
    d_off = C.dev(off)
    roots, roots2 = (torch.empty((n_trees, 4), dtype=torch.int64, device=dev) for _ in range(2))
    d_lv = torch.empty((TS.levels_bound(n_leaves, n_trees, max_leaves, arity) + 1, 4), dtype=torch.int64, device=dev)
    ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, max_leaves, roots, None, arity=arity)   # level-major scratch
    ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, max_leaves, roots2, d_lv, arity=arity)  # tree-major d_levels
    torch.cuda.synchronize()
    assert torch.equal(roots, roots2), "the two builds disagree"
    for k in ks:
        tid = rng.integers(0, n_trees, k)
        lid = (rng.random(k) * sizes[tid]).astype(np.int64)
        pairs = np.unique(tid.astype(np.int64) << 32 | lid)  # the update call wants distinct (tree, leaf) pairs: a pair drawn twice
        tid, lid, k = pairs >> 32, pairs & 0xffffffff, pairs.size  # with two values leaves whichever landed, and its opening may not verify
        d_tid, d_lid = C.dev(tid.astype(np.uint32)), C.dev(lid.astype(np.uint64))
        out = (torch.empty((k, 4), dtype=torch.int64, device=dev), torch.empty((k, D, arity - 1, 4), dtype=torch.int64, device=dev),
               torch.empty((k, D), dtype=torch.uint8, device=dev), torch.empty((k,), dtype=torch.uint8, device=dev))
        back = torch.empty((k, 4), dtype=torch.int64, device=dev)
        ok = torch.zeros((k,), dtype=torch.uint8, device=dev)

        def open_and_verify(what):
            ctx.merkle_forest_ragged_openings_device(d, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, k, out=out, arity=arity)
            ctx.merkle_path_ragged_device(tag, out[0], out[1], out[2], out[3], D, back, k, arity=arity)
            ctx.merkle_forest_ragged_verify_device(tag, out[0], out[1], out[2], out[3], D, d_tid, roots, n_trees, ok, k, arity=arity)
            torch.cuda.synchronize()
            assert int(ok.sum()) == k, "%s: %d of %d openings verify" % (what, int(ok.sum()), k)
            assert torch.equal(back, roots[torch.from_numpy(tid).to(dev)]), what

        open_and_verify("built")
        new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device=dev)
        ctx.merkle_forest_ragged_update_device(tag, d, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, new, k, d_roots=roots, arity=arity)
        open_and_verify("updated")
    print("arity %d, %d trees, %d leaves, depth %d, k = %s: ok" % (arity, n_trees, n_leaves, D, list(ks)))


def run_changes(ctx, arity, sizes, k, seed):
    """a journaled update with its undo and redo, a shared proof of the updated pairs, an append and a resize: each result against a fresh
    build of the forest it should equal"""
    import torch
    from poseidon252_amd import merkle as M
    rng = np.random.default_rng(seed)
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    sizes = np.asarray(sizes, np.int64)
    n_trees, max_leaves = len(sizes), int(sizes.max())
    off = TS.offsets(sizes)
    n_leaves, D = int(off[-1]), TS.depth(max_leaves, arity)
    dev = torch.device("cuda:0")
    d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device=dev)
    d_off = C.dev(off)
    roots = torch.empty((n_trees, 4), dtype=torch.int64, device=dev)
    d_lv = torch.empty((TS.levels_bound(n_leaves, n_trees, max_leaves, arity) + 1, 4), dtype=torch.int64, device=dev)
    ctx.merkle_forest_ragged_device(tag, d, d_off, n_trees, max_leaves, roots, d_lv, arity=arity)

    def fresh_roots(leaves, offsets, trees, top, levels_like):
        out = torch.empty((trees, 4), dtype=torch.int64, device=dev)
        ctx.merkle_forest_ragged_device(tag, leaves, offsets, trees, top, out, torch.empty_like(levels_like), arity=arity)
        torch.cuda.synchronize()
        return out

    tid = rng.integers(0, n_trees, k)
    lid = (rng.random(k) * sizes[tid]).astype(np.int64)
    pairs = np.unique(tid.astype(np.int64) << 32 | lid)  # (distinct pairs: as in run)
    tid, lid, k = pairs >> 32, pairs & 0xffffffff, pairs.size
    d0, roots0 = d.clone(), roots.clone()
    new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device=dev)
    journal = M.forest_ragged_update_journaled(ctx, tag, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots=roots, arity=arity)
    roots1 = roots.clone()
    assert torch.equal(roots1, fresh_roots(d, d_off, n_trees, max_leaves, d_lv)), "journaled update: not the roots of a fresh build"
    assert int(journal.n_bad) == 0 and not torch.equal(roots1, roots0)
    bad = M.forest_ragged_journal_swap(ctx, d, d_off, n_trees, max_leaves, d_lv, journal, d_roots=roots, arity=arity)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(d, d0) and torch.equal(roots, roots0), "undo: not the forest before the update"
    bad = M.forest_ragged_journal_swap(ctx, d, d_off, n_trees, max_leaves, d_lv, journal, d_roots=roots, arity=arity)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(roots, roots1), "redo: not the updated forest"

    def prove(what, leaves, offsets, trees, top, levels, rts, t_ids, l_ids):
        proof = M.forest_ragged_multiproof(ctx, leaves, offsets, trees, top, levels, t_ids, l_ids, arity=arity)
        ok = M.forest_ragged_multiproof_verify(ctx, offsets, leaves.shape[0], trees, top, *proof, rts, arity=arity, tag=tag)
        named = torch.zeros(trees, dtype=torch.bool)
        named[torch.as_tensor(np.unique(t_ids))] = True
        assert torch.equal(ok, named), "%s: %d of %d trees' shared proofs verify" % (what, int(ok.sum()), int(named.sum()))

    prove("updated", d, d_off, n_trees, max_leaves, d_lv, roots, tid, lid)

    # an append to every third tree and two new trees, then a resize that cuts every fifth tree, drops the last two and appends again
    m = np.where(np.arange(n_trees + 2) % 3 == 0, rng.integers(1, 2 * arity + 2, n_trees + 2), 0)
    m[n_trees:] = (1, arity + 1)
    a_off = TS.offsets(m)
    d_add = torch.randint(0, 1 << 60, (int(a_off[-1]), 4), dtype=torch.int64, device=dev)
    top = max_leaves + 2 * (2 * arity + 1)  # (room for both appends: none is refused)
    l2, o2, v2, r2, bad2, _ = M.forest_ragged_append(ctx, tag, d, d_off, n_trees, max_leaves, d_lv, d_add, C.dev(a_off), max_leaves_new=top, arity=arity)
    assert int(bad2) == 0 and torch.equal(r2, fresh_roots(l2, o2, n_trees + 2, top, v2)), "append: not the roots of a fresh build"
    sizes2 = np.concatenate([sizes, [0, 0]]) + m
    prove("appended", l2, o2, n_trees + 2, top, v2, r2, tid, lid)
    keep = np.where(np.arange(n_trees) % 5 == 0, (sizes2[:n_trees] + 1) // 2, -1)
    m3 = m[:n_trees] * (np.arange(n_trees) % 2)
    a3 = TS.offsets(m3)
    l3, o3, v3, r3, bad3, _ = M.forest_ragged_resize(ctx, tag, l2, o2, n_trees + 2, top, v2, C.dev(keep.astype(np.int64)), d_add[:int(a3[-1])], C.dev(a3),
                                                     max_leaves_new=top, arity=arity)
    assert int(bad3) == 0 and torch.equal(r3, fresh_roots(l3, o3, n_trees, top, v3)), "resize: not the roots of a fresh build"
    print("arity %d, %d trees, %d leaves, k = %d: journaled update, undo, redo, shared proofs, append, resize ok" % (arity, n_trees, n_leaves, k))


def run_hash_ragged(ctx, n, max_len):
    import torch
    from poseidon252_amd import hash as H
    lens = 1 + np.arange(n) % max_len
    off = TS.offsets(lens)
    d_in = torch.randint(0, 1 << 60, (int(off[-1]), 4), dtype=torch.int64, device="cuda:0")
    out = torch.empty((n, 1, 4), dtype=torch.int64, device="cuda:0")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ctx.hash_ragged_device(C.dev(H.ragged_tags(H.Domain.Other, 1, max_len)), max_len, d_in, C.dev(off), 1, out, n, d_n_bad=bad)
    torch.cuda.synchronize()
    assert int(bad) == 0
    print("hash_ragged, %d messages of 1 .. %d scalars: ok" % (n, max_len))


def run_tree_families(ctx, arity, n_leaves, k, n_trees, per):
    """root-only tree and equal-size forest; k openings of the stored tree verified in bulk; a shared proof of k leaves, verified"""
    import torch
    from testsupport.device import tree_device
    from poseidon252_amd import levels_len
    from poseidon252_amd import merkle as M
    dev = torch.device("cuda:0")
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    d = torch.randint(0, 1 << 60, (n_leaves, 4), dtype=torch.int64, device=dev)
    root, root2 = (torch.empty(4, dtype=torch.int64, device=dev) for _ in range(2))
    d_lv = torch.empty((levels_len(n_leaves, arity), 4), dtype=torch.int64, device=dev)
    tree_device(ctx, arity, tag, d, n_leaves, root, None)   # root only: the scratch pair
    tree_device(ctx, arity, tag, d, n_leaves, root2, d_lv)  # stored
    f_leaves = torch.randint(0, 1 << 60, (n_trees * per, 4), dtype=torch.int64, device=dev)
    f_roots = torch.empty((n_trees, 4), dtype=torch.int64, device=dev)
    ctx.merkle4_forest_device(tag, f_leaves, n_trees, per, f_roots, arity=arity)
    idx = np.sort(np.random.default_rng(7).permutation(n_leaves)[:k]).astype(np.uint32)
    d_idx = C.dev(idx)
    o_l, o_s, o_p, depth = ctx.merkle4_openings_device(d, n_leaves, d_lv, d_idx, k, arity=arity)
    ok = torch.zeros(k, dtype=torch.uint8, device=dev)
    ctx.merkle_verify_batch_device(tag, o_l, o_s, o_p, depth, root2, ok, k, arity=arity)
    m_l = torch.empty((k, 4), dtype=torch.int64, device=dev)
    m_p = torch.empty((ctx.merkle_multiproof_bound(n_leaves, k, arity=arity), 4), dtype=torch.int64, device=dev)
    m_len = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.merkle_multiproof_device(d, n_leaves, d_lv, d_idx, k, m_l, m_p, m_len, arity=arity)
    m_ok = torch.zeros(1, dtype=torch.uint8, device=dev)
    ctx.merkle_multiproof_verify_device(tag, n_leaves, d_idx, m_l, k, m_p, int(m_len), root2, m_ok, arity=arity)
    torch.cuda.synchronize()
    assert torch.equal(root, root2), "the two tree builds disagree"
    assert int(ok.sum()) == k and int(m_ok) == 1, "%d of %d openings verify, the shared proof: %d" % (int(ok.sum()), k, int(m_ok))
    print("arity %d, tree of %d leaves, k = %d, forest of %d x %d: ok" % (arity, n_leaves, k, n_trees, per))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dispatches", metavar="CSV", help="print the ordered dispatch list of a rocprofv3 kernel trace and exit")
    a = ap.parse_args()
    if a.dispatches:
        return dispatches(a.dispatches)
    import poseidon252_amd as P
    ctx = P.Context(0)
    rng = np.random.default_rng(5)
    small = [1, 2, 3, 5, 17, 64, 65, 300, 1000]                      # level 1: 1,457 / 4 + 9 nodes — the groups throughout
    large = np.floor(np.exp(rng.uniform(0, np.log(4 ** 5 + 1), 3000))).astype(np.int64).clip(1, 4 ** 5)  # level 1 past 8,192 nodes
    for arity in (4, 2):
        run(ctx, arity, small, (50,), 1)
        run(ctx, arity, large, (50, 40000), 2)
    for arity in (4, 2):
        run_changes(ctx, arity, small, 50, 3)
        run_changes(ctx, arity, large, 5000, 4)
    run_hash_ragged(ctx, 200, 40)
    run_hash_ragged(ctx, 70000, 8)                  # past the chip's 65,536 lanes
    for arity in (4, 2):
        run_tree_families(ctx, arity, 1000, 37, 64, 16)
        run_tree_families(ctx, arity, 4 ** 10, 70000, 4096, 4 ** 4)  # first levels past 65,536 nodes: the padded narrow levels too


if __name__ == "__main__":
    sys.exit(main())
