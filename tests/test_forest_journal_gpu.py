"""The journaled leaf update of a ragged forest and the swap that undoes and redoes it (p252_merkle{4,2}_forest_ragged_update_journaled_device_into,
p252_merkle{4,2}_forest_ragged_journal_swap_device_into; csrc/forest_journal.hip) on the GPU: the updated forest against a fresh build and the
oracle, the journal against the numpy model (tests/forestjournal.py) and the bytes from before the update, undo and redo byte for
byte, stacked journals, duplicates and bad updates, edge sizes, a journal swapped into a forest it was not taken on, streams, graph
capture, the C++ mirror, and the swap against the re-update it replaces."""
import os
import time

import numpy as np
import pytest

import forestjournal as FJ
from helpers.forest import SENTINEL, _check_against_fresh_build, _distinct_pairs, _forest, _mix, _np, _open, _tag, _torch, _verify, dirty_count
from helpers.percall import build_cpp_mirror, run_cpp_mirror
from testsupport import treeshape as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_FILL = 0x5A5A5A5A  # no journal id has this tree id, level and index


def _bound(ctx, arity, n_leaves, n_trees, max_leaves, k):
    return getattr(ctx, "merkle%d_forest_ragged_journal_bound" % arity)(n_leaves, n_trees, max_leaves, k)


def _journaled(ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots=None, cap=None):
    """one journaled update into a sentinel-filled journal -> dict(ids, values, len, bad, hashed, cap), device tensors"""
    import torch
    k = len(tid)
    if cap is None:
        cap = _bound(ctx, arity, d.shape[0], n_trees, max_leaves, k)
    J = dict(ids=torch.full((cap, 4), ID_FILL, dtype=torch.int32, device=d.device),
             values=torch.full((cap, 4), SENTINEL, dtype=torch.int64, device=d.device),
             len=torch.full((1,), -7, dtype=torch.int64, device=d.device),  # (the call sets it)
             bad=torch.zeros(1, dtype=torch.int32, device=d.device), hashed=torch.zeros(1, dtype=torch.int64, device=d.device), cap=cap)
    call = getattr(ctx, "merkle%d_forest_ragged_update_journaled_device" % arity)
    call(_tag(arity), d, d_off, n_trees, max_leaves, d_lv, _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64)), _torch(new), k,
         J["ids"], J["values"], cap, J["len"], d_roots=d_roots, d_n_bad=J["bad"], d_n_hashed=J["hashed"])
    return J


def _swap(ctx, arity, d, d_off, n_trees, max_leaves, d_lv, J, d_roots=None):
    """one swap -> n_bad (a device tensor)"""
    import torch
    bad = torch.zeros(1, dtype=torch.int32, device=d.device)
    getattr(ctx, "merkle%d_forest_ragged_journal_swap_device" % arity)(d, d_off, n_trees, max_leaves, d_lv, J["ids"], J["values"], J["cap"], J["len"],
                                                                       d_roots=d_roots, d_n_bad=bad)
    return bad


def _lo(sizes, arity):
    from poseidon252_amd import levels_len
    return np.concatenate([[0], np.cumsum([levels_len(int(n), arity) if n > 0 else 0 for n in sizes])]).astype(np.int64)


def _node_rows(entries, sizes, off, arity):
    """for [(tree, level, node)]: (is a leaf, the row in the flat leaves or in d_levels)"""
    lo = _lo(sizes, arity)
    rows = []
    for t, level, i in entries:
        counts = [int(sizes[t])] + TS.level_widths(sizes[t], arity)
        rows.append((level == 0, int(off[t]) + i if level == 0 else int(lo[t]) + sum(counts[1:level]) + i))
    return rows


def _mixed(gpu_ctx, oracle_mod, arity, seed):
    """the forest of the issue: _mix(arity) * 2 shuffled, offsets[0] != 0, sentinel-filled levels with a tail"""
    sizes = _mix(arity) * 2
    np.random.default_rng(arity).shuffle(sizes)
    off = TS.offsets(sizes, start=5)
    flat = oracle_mod.fill_random(seed + arity, int(off[-1]) + 3)
    return sizes, off, flat, _forest(gpu_ctx, arity, flat, off)


def _sentinel_roots(n_trees, device):
    import torch
    return torch.full((n_trees, 4), SENTINEL, dtype=torch.int64, device=device)


def _state(d, d_lv, d_roots):
    return d.clone(), d_lv.clone(), d_roots.clone()


def _same(state, d, d_lv, d_roots):
    import torch
    return torch.equal(state[0], d) and torch.equal(state[1], d_lv) and torch.equal(state[2], d_roots)


# ---- 1. parity, and the journal against the model ----
@pytest.mark.parametrize("arity", [4, 2])
def test_parity_and_the_journal_holds_what_was_overwritten(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1A00)
    torch.cuda.synchronize()
    before_lv = _np(d_lv)
    untouched = [0, 5, len(sizes) - 1, int(np.argmax(sizes))]
    tid, lid = _distinct_pairs(sizes, np.random.default_rng(41 + arity), 500, [t for t in range(len(sizes)) if t not in untouched])
    assert tid.size == 500  # not a multiple of 64
    new = oracle_mod.fill_random(0x1A10 + arity, 500)
    d_roots = _sentinel_roots(len(sizes), d.device)
    J = _journaled(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    want_hashed = dirty_count(sizes, tid, lid, arity)
    assert int(J["bad"]) == 0 and int(J["hashed"]) == want_hashed and int(J["len"]) == 500 + want_hashed
    _check_against_fresh_build(gpu_ctx, oracle_mod, arity, flat, off, tid, lid, new, d, d_lv, d_roots)
    n = int(J["len"])
    got = FJ.ids_to_tuples(_np(J["ids"])[:n])
    assert len(set(got)) == n and set(got) == FJ.journal_entries(sizes, arity, tid, lid)
    levels = [e[1] for e in got]
    assert levels == sorted(levels) and levels[:500] == [0] * 500  # the leaves first, then level by level
    values = _np(J["values"])
    for g, (leaf, row) in enumerate(_node_rows(got, sizes, off, arity)):
        assert np.array_equal(values[g], flat[row] if leaf else before_lv[row]), (g, got[g])
    # nothing past the length
    assert bool((J["ids"][n:] == ID_FILL).all()) and bool((J["values"][n:] == SENTINEL).all()) and n < J["cap"]


# ---- 2. undo and redo ----
@pytest.mark.parametrize("arity", [4, 2])
def test_one_swap_undoes_and_a_second_redoes_byte_for_byte(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1B00)
    n_trees, max_leaves = len(sizes), max(sizes)
    untouched = [1, 7, int(np.argmax(sizes))]
    tid, lid = _distinct_pairs(sizes, np.random.default_rng(51 + arity), 500, [t for t in range(n_trees) if t not in untouched])
    touched = sorted(set(tid.tolist()))
    new = oracle_mod.fill_random(0x1B10 + arity, tid.size)
    d_roots = _sentinel_roots(n_trees, d.device)
    pre = _state(d, d_lv, d_roots)
    J = _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots)
    post = _state(d, d_lv, d_roots)
    ids, length = J["ids"].clone(), J["len"].clone()
    J["hashed"].zero_()
    for want_leaves, want_lv, want_roots, leaves_np in ((pre[0], pre[1], roots, flat[off[tid].astype(np.int64) + lid]), (post[0], post[1], post[2], new)):
        bad = _swap(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, J, d_roots)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(J["hashed"]) == 0
        assert torch.equal(d, want_leaves) and torch.equal(d_lv, want_lv)  # (the whole of d_levels: nothing past the used length is written)
        assert torch.equal(d_roots[touched], want_roots[touched]) and bool((d_roots[untouched] == SENTINEL).all())
        assert torch.equal(J["ids"], ids) and torch.equal(J["len"], length)
        o = _open(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid)
        ok = _verify(gpu_ctx, arity, o, d_roots, n_trees)
        torch.cuda.synchronize()
        assert np.array_equal(_np(o["leaves"]), leaves_np) and _np(ok).tolist() == [1] * tid.size
    assert not torch.equal(pre[0], post[0]) and not torch.equal(pre[1], post[1])


# ---- 3. journals stack ----
@pytest.mark.parametrize("arity", [4, 2])
def test_journals_stack(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1C00)
    n_trees, max_leaves = len(sizes), max(sizes)
    rng = np.random.default_rng(61 + arity)
    tid_a, lid_a = _distinct_pairs(sizes, rng, 200)
    tid_b, lid_b = _distinct_pairs(sizes, rng, 200)
    tid_b[:40], lid_b[:40] = tid_a[:40], lid_a[:40]  # the same leaves in both ...
    tid_b[40:80], lid_b[40:80] = tid_a[40:80], lid_a[40:80] ^ 1  # ... and neighbours under the same parents
    keep = lid_b < np.asarray(sizes)[tid_b]
    tid_b, lid_b = np.unique(np.stack([tid_b[keep], lid_b[keep]], axis=1), axis=0).T
    new_a, new_b = oracle_mod.fill_random(0x1C10 + arity, tid_a.size), oracle_mod.fill_random(0x1C20 + arity, tid_b.size)
    d_roots = roots.clone()
    s0 = _state(d, d_lv, d_roots)
    A = _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid_a, lid_a, new_a, d_roots)
    s1 = _state(d, d_lv, d_roots)
    B = _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid_b, lid_b, new_b, d_roots)
    s2 = _state(d, d_lv, d_roots)
    torch.cuda.synchronize()
    shared = FJ.journal_entries(sizes, arity, tid_a, lid_a) & FJ.journal_entries(sizes, arity, tid_b, lid_b)
    assert len(shared) > 80 and any(e[1] == 0 for e in shared)
    for J, want in ((B, s1), (A, s0), (A, s1), (B, s2)):
        assert int(_swap(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, J, d_roots)) == 0
        assert _same(want, d, d_lv, d_roots)
    want = flat.copy()
    want[off[tid_a].astype(np.int64) + lid_a] = new_a
    want[off[tid_b].astype(np.int64) + lid_b] = new_b
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv)


# ---- 4. duplicates and bad updates ----
@pytest.mark.parametrize("arity", [4, 2])
def test_duplicates_are_applied_once_and_bad_updates_counted(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1D00)
    n_trees, max_leaves = len(sizes), max(sizes)
    big, mid = int(np.argmax(sizes)), sizes.index(65)
    base_t, base_l = _distinct_pairs(sizes, np.random.default_rng(71 + arity), 90, [t for t in range(n_trees) if t not in (big, mid)])
    tid = np.concatenate([base_t, [big, big, big], [mid, mid], [n_trees], [mid]])
    lid = np.concatenate([base_l, [17, 17, 17], [64, 64], [0], [sizes[mid]]])  # (leaf id = n_t last)
    new = oracle_mod.fill_random(0x1D10 + arity, tid.size)
    new[94] = new[93]  # the pair given twice carries one value
    order = np.random.default_rng(arity).permutation(tid.size)
    tid, lid, new = tid[order], lid[order], new[order]
    trio = new[(tid == big) & (lid == 17)]
    assert trio.shape[0] == 3 and len({r.tobytes() for r in trio}) == 3
    d_roots = roots.clone()
    pre = _state(d, d_lv, d_roots)
    J = _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    good = (tid < n_trees) & (lid < np.asarray(sizes + [0])[np.minimum(tid, n_trees)])
    n_distinct = 90 + 2
    assert int(J["bad"]) == 2 and int(J["hashed"]) == dirty_count(sizes, tid[good], lid[good], arity)
    assert int(J["len"]) == n_distinct + int(J["hashed"])
    got = FJ.ids_to_tuples(_np(J["ids"])[:int(J["len"])])
    assert len(set(got)) == len(got) and set(got) == FJ.journal_entries(sizes, arity, tid, lid)
    stored = _np(d)
    landed = stored[int(off[big]) + 17]
    assert any(np.array_equal(landed, r) for r in trio)  # one of the three, whole
    assert np.array_equal(stored[int(off[mid]) + 64], new[(tid == mid) & (lid == 64)][0])
    want = flat.copy()
    want[off[tid[good]].astype(np.int64) + lid[good]] = new[good]
    want[int(off[big]) + 17] = landed
    assert np.array_equal(stored, want)
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, stored, off)
    torch.cuda.synchronize()
    assert torch.equal(d_lv, f_lv) and torch.equal(d_roots, f_roots)  # the forest equals a fresh build of what is stored
    assert int(_swap(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, J, d_roots)) == 0
    assert _same(pre, d, d_lv, d_roots)


# ---- 5. edges ----
P_LIMBS = np.array([0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48], dtype=np.uint64)  # the field's modulus


@pytest.mark.parametrize("arity", [4, 2])
def test_a_forest_of_one_leaf_trees(gpu_ctx, oracle_mod, arity):
    """depth 0, d_levels NULL: the root is the leaf REDUCED, after the update and after the swap"""
    import torch
    n_trees = 50
    flat = oracle_mod.fill_random(0x1E00 + arity, n_trees)
    flat[3] = P_LIMBS + np.array([7, 0, 0, 0], dtype=np.uint64)  # limbs >= p
    d, d_off = _torch(flat), _torch(TS.offsets([1] * n_trees))
    built = _sentinel_roots(n_trees, d.device)
    gpu_ctx.merkle_forest_ragged_device(_tag(arity), d, d_off, n_trees, 1, built, None, None, arity=arity)
    tid, lid = np.array([3, 49, 0, 50, 11]), np.array([0, 0, 0, 0, 1])  # (two bad ones)
    new = oracle_mod.fill_random(0x1E10 + arity, tid.size)
    new[1] = P_LIMBS + np.array([9, 0, 0, 0], dtype=np.uint64)
    want = flat.copy()
    want[[3, 49, 0]] = new[:3]
    after = _sentinel_roots(n_trees, d.device)
    gpu_ctx.merkle_forest_ragged_device(_tag(arity), _torch(want), d_off, n_trees, 1, after, None, None, arity=arity)
    d_roots = _sentinel_roots(n_trees, d.device)
    J = _journaled(gpu_ctx, arity, d, d_off, n_trees, 1, None, tid, lid, new, d_roots)
    torch.cuda.synchronize()
    assert J["cap"] == 5 and int(J["bad"]) == 2 and int(J["hashed"]) == 0 and int(J["len"]) == 3
    assert np.array_equal(_np(d), want) and torch.equal(d_roots[[3, 49, 0]], after[[3, 49, 0]])
    assert not np.array_equal(_np(d_roots)[49], new[1]) and _np(d_roots)[49].tolist() == [9, 0, 0, 0]  # reduced; the leaf keeps its bytes
    assert int((d_roots == SENTINEL).all(dim=1).sum()) == n_trees - 3
    assert set(FJ.ids_to_tuples(_np(J["ids"])[:3])) == {(3, 0, 0), (49, 0, 0), (0, 0, 0)}
    assert int(_swap(gpu_ctx, arity, d, d_off, n_trees, 1, None, J, d_roots)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(d), flat) and torch.equal(d_roots[[3, 49, 0]], built[[3, 49, 0]])
    assert _np(d_roots)[3].tolist() == [7, 0, 0, 0] and np.array_equal(_np(d)[3], flat[3])
    assert int((d_roots == SENTINEL).all(dim=1).sum()) == n_trees - 3
    assert int(_swap(gpu_ctx, arity, d, d_off, n_trees, 1, None, J, d_roots)) == 0
    assert np.array_equal(_np(d), want) and torch.equal(d_roots[[3, 49, 0]], after[[3, 49, 0]])


@pytest.mark.parametrize("arity", [4, 2])
def test_one_update_a_short_journal_and_a_long_one(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1E20)
    n_trees, max_leaves = len(sizes), max(sizes)
    big = int(np.argmax(sizes))
    d_roots = roots.clone()
    pre = _state(d, d_lv, d_roots)
    new = oracle_mod.fill_random(0x1E30 + arity, 1)
    bound = _bound(gpu_ctx, arity, d.shape[0], n_trees, max_leaves, 1)
    assert bound == 1 + TS.depth(max_leaves, arity)
    # one entry short: refused, nothing enqueued, nothing changes
    with pytest.raises(ValueError, match="journal_cap %d is below the call's bound of %d" % (bound - 1, bound)):
        _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, [big], [sizes[big] - 1], new, d_roots, cap=bound - 1)
    torch.cuda.synchronize()
    assert _same(pre, d, d_lv, d_roots)
    # k = 1, a journal longer than needed: the entries past the length keep the sentinel
    J = _journaled(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, [big], [sizes[big] - 1], new, d_roots, cap=bound + 7)
    torch.cuda.synchronize()
    n = int(J["len"])
    assert n == bound and int(J["hashed"]) == bound - 1 and int(J["bad"]) == 0
    assert bool((J["ids"][n:] == ID_FILL).all()) and bool((J["values"][n:] == SENTINEL).all())
    _check_against_fresh_build(gpu_ctx, oracle_mod, arity, flat, off, [big], [sizes[big] - 1], new, d, d_lv,
                               torch.where(torch.arange(n_trees, device=d.device)[:, None] == big, d_roots, SENTINEL))
    assert int(_swap(gpu_ctx, arity, d, d_off, n_trees, max_leaves, d_lv, J, d_roots)) == 0
    assert _same(pre, d, d_lv, d_roots)
    assert bool((J["ids"][n:] == ID_FILL).all()) and bool((J["values"][n:] == SENTINEL).all())


@pytest.mark.parametrize("arity", [4, 2])
def test_one_wide_tree_both_digest_kernels_and_multi_block_appends(gpu_ctx, oracle_mod, arity):
    """k = 20,000 distinct leaves of one tree: the level lists pass 8,192 and 16,384 records"""
    import torch
    n = 4 ** 8 if arity == 4 else 2 ** 16
    off = TS.offsets([n], start=1)
    flat = oracle_mod.fill_random(0x1E40 + arity, n + 1)
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
    lid = np.random.default_rng(81 + arity).choice(n, 20000, replace=False)
    tid = np.zeros(lid.size, np.int64)
    new = oracle_mod.fill_random(0x1E50 + arity, lid.size)
    pre = _state(d, d_lv, roots)
    J = _journaled(gpu_ctx, arity, d, d_off, 1, n, d_lv, tid, lid, new, roots)
    torch.cuda.synchronize()
    want_hashed = dirty_count([n], tid, lid, arity)
    lists = [len({i // arity ** l for i in lid.tolist()}) for l in range(0, 4)]  # the records of lists 0 .. 3
    assert max(lists) > 16384 and any(8192 < x <= 16384 for x in lists), lists  # (what the case is for)
    assert int(J["bad"]) == 0 and int(J["hashed"]) == want_hashed and int(J["len"]) == 20000 + want_hashed
    want = flat.copy()
    want[1 + lid] = new
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
    torch.cuda.synchronize()
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots)
    got = FJ.ids_to_tuples(_np(J["ids"])[:int(J["len"])])
    assert len(set(got)) == len(got) and set(got) == FJ.journal_entries([n], arity, tid, lid)
    assert int(_swap(gpu_ctx, arity, d, d_off, 1, n, d_lv, J, roots)) == 0
    assert _same(pre, d, d_lv, roots)
    assert int(_swap(gpu_ctx, arity, d, d_off, 1, n, d_lv, J, roots)) == 0
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots)


# ---- 6. a journal that was not taken on this forest ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_foreign_journal_writes_only_what_names_a_node_of_the_forest(gpu_ctx, oracle_mod, arity):
    import torch
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x1F00)
    rng = np.random.default_rng(91 + arity)
    tid, lid = (np.concatenate(x) for x in zip(_distinct_pairs(sizes, rng, 30, [0, 1, 2]), _distinct_pairs(sizes, rng, 470, range(3, len(sizes)))))
    J = _journaled(gpu_ctx, arity, d, d_off, len(sizes), max(sizes), d_lv, tid, lid, oracle_mod.fill_random(0x1F10 + arity, tid.size))
    # the first three trees alone, with their own max_leaves
    small = sizes[:3]
    s_off = TS.offsets(small, start=5)
    s_flat = flat[:int(s_off[-1]) + 3].copy()
    sd, sd_off, s_roots, sd_lv = _forest(gpu_ctx, arity, s_flat, s_off)
    torch.cuda.synchronize()
    n = int(J["len"])
    # two hand-made ids in the journal's unused tail: level = depth + 2 of tree 0, and node index = the count of tree 2's level 1
    t2 = [small[2]] + TS.level_widths(small[2], arity)
    hand = np.array([[0, TS.depth(small[0], arity) + 2 + 1, 0, 0], [2, 1 + 1 if len(t2) > 1 else 1, t2[1] if len(t2) > 1 else t2[0], 0]], np.uint32)
    assert n + 2 <= J["cap"]
    J["ids"][n:n + 2] = _torch(hand)
    J["len"] += 2
    ids, values = _np(J["ids"]).copy(), _np(J["values"]).copy()
    used = int(_lo(small, arity)[-1])
    e_leaves, e_lv, e_values, e_roots = s_flat.copy(), FJ.split_levels(_np(sd_lv)[:used], small, arity), values.copy(), _np(s_roots).copy()
    reduce = lambda x: x  # noqa: E731 (the leaves here are below the modulus)
    e_bad = FJ.swap_host(e_leaves, s_off, small, e_lv, ids.view(np.uint32), e_values, n + 2, arity, e_roots, reduce)
    fits = sum(1 for t, level, i in FJ.ids_to_tuples(ids[:n]) if t < 3)
    assert e_bad == 2 + (n - fits) and 0 < fits < n
    tail_before = sd_lv[used:].clone()
    bad = _swap(gpu_ctx, arity, sd, sd_off, 3, max(small), sd_lv, J, s_roots)
    torch.cuda.synchronize()
    assert int(bad) == e_bad
    assert np.array_equal(_np(sd), e_leaves) and np.array_equal(_np(sd_lv)[:used], np.concatenate([x for x in e_lv if len(x)] or [np.zeros((0, 4), np.uint64)]))
    assert torch.equal(sd_lv[used:], tail_before) and bool((sd_lv[used:] == SENTINEL).all())
    assert np.array_equal(_np(J["values"]), e_values) and np.array_equal(_np(J["ids"]), ids)  # the skipped entries keep their values
    assert np.array_equal(_np(s_roots), e_roots)


# ---- 7. streams and capture ----
@pytest.mark.parametrize("arity", [4, 2])
def test_update_and_swap_captured_on_one_stream(gpu_ctx, oracle_mod, arity):
    import torch
    sizes = [1, 5, 17, 256, 1000, 3, 64] * 20
    off = TS.offsets(sizes)
    flat = oracle_mod.fill_random(0x2000 + arity, int(off[-1]))
    d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
    n_trees, max_leaves, k = len(sizes), 1000, 3000
    tid, lid = _distinct_pairs(sizes, np.random.default_rng(arity), k)
    d_tid, d_lid = _torch(tid.astype(np.uint32)), _torch(lid.astype(np.uint64))
    d_new = _torch(oracle_mod.fill_random(0x2010 + arity, k))
    cap = _bound(gpu_ctx, arity, d.shape[0], n_trees, max_leaves, k)
    ids = torch.zeros((cap, 4), dtype=torch.int32, device=d.device)
    values = torch.zeros((cap, 4), dtype=torch.int64, device=d.device)
    jlen = torch.zeros(1, dtype=torch.int64, device=d.device)
    bad = torch.zeros(2, dtype=torch.int32, device=d.device)
    mid = [t.clone() for t in (d, d_lv, roots)]  # the forest between the two calls, copied inside the graph
    tag = _tag(arity)
    upd = getattr(gpu_ctx, "merkle%d_forest_ragged_update_journaled_device" % arity)
    swp = getattr(gpu_ctx, "merkle%d_forest_ragged_journal_swap_device" % arity)

    def both():
        upd(tag, d, d_off, n_trees, max_leaves, d_lv, d_tid, d_lid, d_new, k, ids, values, cap, jlen, d_roots=roots, d_n_bad=bad[:1])
        for dst, src in zip(mid, (d, d_lv, roots)):
            dst.copy_(src)
        swp(d, d_off, n_trees, max_leaves, d_lv, ids, values, cap, jlen, d_roots=roots, d_n_bad=bad[1:])
    pre = _state(d, d_lv, roots)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        both()  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    assert _same(pre, d, d_lv, roots)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        both()
    for rep in range(2):
        new = oracle_mod.fill_random(0x2020 + arity + 16 * rep, k)
        d_new.copy_(_torch(new))
        bad.zero_()
        jlen.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert _same(pre, d, d_lv, roots) and _np(bad).tolist() == [0, 0], rep  # each replay leaves the original forest
        assert int(jlen) == k + dirty_count(sizes, tid, lid, arity)
        want = flat.copy()
        want[off[tid].astype(np.int64) + lid] = new
        _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
        torch.cuda.synchronize()
        assert np.array_equal(_np(mid[0]), want) and torch.equal(mid[1], f_lv) and torch.equal(mid[2], f_roots), rep


def test_two_streams_of_one_context(gpu_ctx, oracle_mod):
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for j, (arity, sizes) in enumerate(((4, [3000, 7, 900, 1] * 10), (2, [65, 1024, 2, 300] * 10))):
        off = TS.offsets(sizes)
        flat = oracle_mod.fill_random(0x2100 + j, int(off[-1]))
        tid, lid = _distinct_pairs(sizes, np.random.default_rng(j), 6000)
        new = oracle_mod.fill_random(0x2110 + j, tid.size)
        n, m = len(sizes), max(sizes)
        # serially, on the default stream
        d, d_off, roots, d_lv = _forest(gpu_ctx, arity, flat, off)
        pre = _state(d, d_lv, roots)
        S = _journaled(gpu_ctx, arity, d, d_off, n, m, d_lv, tid, lid, new, roots)
        post = _state(d, d_lv, roots)
        torch.cuda.synchronize()
        d2, d2_off, roots2, d2_lv = _forest(gpu_ctx, arity, flat, off)
        jobs.append(dict(arity=arity, n=n, m=m, d=d2, d_off=d2_off, roots=roots2, d_lv=d2_lv, tid=tid, lid=lid, new=new, pre=pre, post=post,
                         serial=set(FJ.ids_to_tuples(_np(S["ids"])[:int(S["len"])])), serial_len=int(S["len"])))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for rep in range(3):
        for J, s in zip(jobs, streams):
            with torch.cuda.stream(s):
                J["j"] = _journaled(gpu_ctx, J["arity"], J["d"], J["d_off"], J["n"], J["m"], J["d_lv"], J["tid"], J["lid"], J["new"], J["roots"])
                J["mid"] = _state(J["d"], J["d_lv"], J["roots"])
                J["bad"] = _swap(gpu_ctx, J["arity"], J["d"], J["d_off"], J["n"], J["m"], J["d_lv"], J["j"], J["roots"])
        torch.cuda.synchronize()
        for J in jobs:
            assert _same(J["post"], *J["mid"]) and _same(J["pre"], J["d"], J["d_lv"], J["roots"]), (rep, J["arity"])
            assert int(J["bad"]) == 0 and int(J["j"]["len"]) == J["serial_len"]
            assert set(FJ.ids_to_tuples(_np(J["j"]["ids"])[:J["serial_len"]])) == J["serial"]


# ---- 8. the conveniences and the C++ mirror ----
@pytest.mark.parametrize("arity", [4, 2])
def test_merkle_conveniences_round_trip(gpu_ctx, oracle_mod, arity):
    import torch
    from poseidon252_amd import merkle as M
    sizes, off, flat, (d, d_off, roots, d_lv) = _mixed(gpu_ctx, oracle_mod, arity, 0x2200)
    n_trees, max_leaves = len(sizes), max(sizes)
    tid, lid = _distinct_pairs(sizes, np.random.default_rng(arity), 77)
    new = oracle_mod.fill_random(0x2210 + arity, 77)
    pre = _state(d, d_lv, roots)
    j = M.forest_ragged_update_journaled(gpu_ctx, None, d, d_off, n_trees, max_leaves, d_lv, tid, lid, new, d_roots=roots, arity=arity)
    assert j.cap == _bound(gpu_ctx, arity, d.shape[0], n_trees, max_leaves, 77)
    assert int(j.n_bad) == 0 and int(j.len) == 77 + int(j.n_hashed) and int(j.n_hashed) == dirty_count(sizes, tid, lid, arity)
    want = flat.copy()
    want[off[tid].astype(np.int64) + lid] = new
    _, _, f_roots, f_lv = _forest(gpu_ctx, arity, want, off)
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots)
    assert int(M.forest_ragged_journal_swap(gpu_ctx, d, d_off, n_trees, max_leaves, d_lv, j, d_roots=roots, arity=arity)) == 0
    assert _same(pre, d, d_lv, roots)
    assert int(M.forest_ragged_journal_swap(gpu_ctx, d, d_off, n_trees, max_leaves, d_lv, j, d_roots=roots, arity=arity)) == 0
    assert np.array_equal(_np(d), want) and torch.equal(d_lv, f_lv) and torch.equal(roots, f_roots)


def test_cpp_mirror_on_gpu(gpu_ctx, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_journal_api", tmp_path, oracle=False))


# ---- 9. the swap against what it replaces ----
def _median_ms(fn, reps, warm):
    import torch
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def test_the_swap_is_faster_than_the_re_update_with_the_old_leaves(gpu_ctx):
    """one 4^8-leaf tree, k = 2^14 distinct leaves, medians of 7 after 2 warm-ups: the re-update launches eight digest levels of at
    least a lone wave's latency each (0.11-0.12 ms, README), the swap launches none.  No ratio is asserted."""
    import torch
    n, k = 4 ** 8, 1 << 14
    d = torch.randint(0, 1 << 60, (n, 4), dtype=torch.int64, device="cuda:0")
    d_off = _torch(TS.offsets([n]))
    roots = torch.zeros((1, 4), dtype=torch.int64, device="cuda:0")
    d_lv = torch.zeros((n // 3 + 8 + 1, 4), dtype=torch.int64, device="cuda:0")
    tag = _tag(4)
    gpu_ctx.merkle_forest_ragged_device(tag, d, d_off, 1, n, roots, d_lv, None, arity=4)
    lid = np.random.default_rng(1).choice(n, k, replace=False)
    d_tid, d_lid = _torch(np.zeros(k, np.uint32)), _torch(lid.astype(np.uint64))
    d_old = d[_torch(lid.astype(np.int64))].clone()
    d_new = torch.randint(0, 1 << 60, (k, 4), dtype=torch.int64, device="cuda:0")
    cap = gpu_ctx.merkle4_forest_ragged_journal_bound(n, 1, n, k)
    ids, values = torch.zeros((cap, 4), dtype=torch.int32, device="cuda:0"), torch.zeros((cap, 4), dtype=torch.int64, device="cuda:0")
    jlen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    pre = _state(d, d_lv, roots)
    gpu_ctx.merkle4_forest_ragged_update_journaled_device(tag, d, d_off, 1, n, d_lv, d_tid, d_lid, d_new, k, ids, values, cap, jlen, d_roots=roots)
    swap = lambda: gpu_ctx.merkle4_forest_ragged_journal_swap_device(d, d_off, 1, n, d_lv, ids, values, cap, jlen, d_roots=roots)  # noqa: E731
    old = lambda: gpu_ctx.merkle_forest_ragged_update_device(tag, d, d_off, 1, n, d_lv, d_tid, d_lid, d_old, k, d_roots=roots)  # noqa: E731
    t_swap = _median_ms(swap, 7, 2)  # (an odd number of swaps in all: the forest is the one before the update)
    torch.cuda.synchronize()
    assert _same(pre, d, d_lv, roots)
    swap()  # redo, so that the re-update has the update's work to do
    t_old = _median_ms(old, 7, 2)
    assert _same(pre, d, d_lv, roots)
    print("4^8 leaves, k = 2^14: swap %.3f ms, re-update with the old leaves %.3f ms (%d journal entries)" % (t_swap, t_old, int(jlen)))
    assert t_swap < t_old, "swap %.3f ms vs re-update %.3f ms" % (t_swap, t_old)
