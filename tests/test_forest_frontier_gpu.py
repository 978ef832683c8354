"""A forest of append-only Merkle trees kept only as their frontiers (p252_merkle{4,2}_forest_frontier_append_device_into and
_extract_device_into; csrc/forest_frontier.hip) on the GPU.  The reference of every comparison is the oracle's build of ALL leaves a
tree was given so far — its root, and its frontier as the numpy model cuts it out of the full build (testsupport/forestfrontier.py,
checked without a GPU) — never the call itself: every (n, m) transition in one call; both digest kernels; streaming into one tree;
agreement with the stored append; refused appends; unreduced leaves; more trees than one trip of the scan's tile loop; a side stream."""
import os
import re

import numpy as np
import pytest

import edgecases as E
from testsupport import forestfrontier as FF
from testsupport import treeshape as TS
from testsupport.device import tree_device
from helpers.forest import Grown, Old, _append as _stored_append, _np, _outputs, _tag, _torch, _tree
from helpers.percall import build_cpp_mirror, run_cpp_mirror

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
# the scan over the trees is the stored append's: its block and its tile
BLOCK = int(re.search(r"FA_BLOCK = (\d+);", open(os.path.join(_CSRC, "forest_append.hip")).read()).group(1))
SCAN_TILE = int(re.search(r"FOREST_APPEND_SCAN_TILE = (\d+);", open(os.path.join(_CSRC, "forest_append.h")).read()).group(1))
assert "forest_append_scan_sum_rule" in open(os.path.join(_CSRC, "forest_frontier.hip")).read()


class Dev:
    """a frontier state on the device, all zero: a forest of empty trees"""

    def __init__(self, ctx, arity, n_trees, max_leaves):
        import torch
        self.ctx, self.arity, self.n_trees, self.max_leaves = ctx, arity, n_trees, max_leaves
        self.bound = FF.bound(max_leaves, arity)
        assert self.bound == (ctx.merkle4_forest_frontier_bound if arity == 4 else ctx.merkle2_forest_frontier_bound)(max_leaves)
        self.counts = torch.zeros(n_trees, dtype=torch.int64, device="cuda:0")
        self.frontier = torch.zeros((n_trees, self.bound, 4), dtype=torch.int64, device="cuda:0")
        self.roots = torch.zeros((n_trees, 4), dtype=torch.int64, device="cuda:0")

    def append(self, d_add, d_aoff, bad=None, hashed=None):
        call = self.ctx.merkle4_forest_frontier_append_device if self.arity == 4 else self.ctx.merkle2_forest_frontier_append_device
        call(_tag(self.arity), self.counts, self.frontier, self.roots, self.n_trees, self.max_leaves, d_add, d_aoff, bad, hashed)

    def extract(self, old, bad=None):
        call = self.ctx.merkle4_forest_frontier_extract_device if self.arity == 4 else self.ctx.merkle2_forest_frontier_extract_device
        call(old.d, old.d_off, old.n_trees, old.max_leaves, old.d_lv, old.roots, self.max_leaves, self.counts, self.frontier, self.roots, bad)

    def numpy(self):
        import torch
        torch.cuda.synchronize()
        return _np(self.counts).astype(np.int64), _np(self.frontier), _np(self.roots)


def _counters():
    import torch
    return torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0")


def _want_one(oracle_mod, arity, leaves, max_leaves):
    """(rows (bound, 4), root) of a tree of these leaves, from the oracle's full build; no leaf: all zero"""
    n = leaves.shape[0]
    if n == 0:
        return np.zeros((FF.bound(max_leaves, arity), 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    if n > 4096:  # (level by level on the oracle's threads)
        root, levels = E.oracle_tree(_tag(arity), leaves, arity)
    else:
        root, levels = _tree(oracle_mod, arity)(_tag(arity), leaves, want_levels=True)[:2]
    return FF.frontier_of(leaves, levels, n, arity, max_leaves).reshape(-1, 4), root


def _want(oracle_mod, arity, trees, max_leaves):
    """the state of the forest whose trees hold these leaves: (counts, frontier (T, bound, 4), roots (T, 4))"""
    both = E._pmap(lambda lv: _want_one(oracle_mod, arity, lv, max_leaves), trees)
    return np.array([t.shape[0] for t in trees], dtype=np.int64), np.array([b[0] for b in both]), np.array([b[1] for b in both])


def _same(state, want, what=""):
    for name, got, ref in zip(("counts", "frontier", "roots"), state.numpy(), want):
        differ = np.nonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))[0]
        assert differ.size == 0, (what, name, differ[:8].tolist())


def _split(flat, sizes):
    off = TS.offsets(sizes, dtype=np.int64)
    return [flat[off[t]:off[t + 1]] for t in range(len(sizes))]


# ---- 1. every transition in one call ----
@pytest.mark.parametrize("arity", [4, 2])
def test_every_transition_in_one_call(gpu_ctx, oracle_mod, arity):
    """all (n, m) with 0 <= n <= 70, 0 <= m <= 20 as the trees of one forest: every digit carry, depth growth, n = A^k, n = 0, n' = 1,
    m = 0; the starting state is the extraction from a built forest, itself compared with the model"""
    pairs = [(n, m) for n in range(71) for m in range(21)]
    assert len(pairs) == 1491
    np.random.default_rng(arity).shuffle(pairs)
    sizes, adds = [p[0] for p in pairs], [p[1] for p in pairs]
    flat = oracle_mod.fill_random(0xF00 + arity, sum(sizes))
    add = oracle_mod.fill_random(0xF10 + arity, sum(adds))
    old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), 70)
    st = Dev(gpu_ctx, arity, len(pairs), 90)
    st.frontier.fill_(-1), st.roots.fill_(-1), st.counts.fill_(-1)  # (the extraction writes every byte of the state)
    bad, hashed = _counters()
    st.extract(old, bad)
    before, grow = _split(flat, sizes), _split(add, adds)
    _same(st, _want(oracle_mod, arity, before, 90), "extract")
    assert int(bad) == 21  # the trees without a leaf: bad to the build, empty here
    bad.zero_()
    st.append(_torch(add), _torch(TS.offsets(adds)), bad, hashed)
    _same(st, _want(oracle_mod, arity, [np.concatenate(p) for p in zip(before, grow)], 90), "append")
    assert int(bad) == 0 and int(hashed) == sum(FF.n_hashed(n, m, arity) for n, m in pairs)


# ---- 2. both digest builds ----
@pytest.mark.parametrize("arity", [4, 2])
def test_a_level_too_wide_for_the_lane_groups_beside_narrow_trees(gpu_ctx, oracle_mod, arity):
    """one tree of 4^8 + 7 (arity 2: 2^16 + 7) leaves gains 3 * 2^16 + 5 beside 300 trees that gain 0 to 3: level 1's list is bounded by
    more than 8,192 nodes, so the one-lane digest kernel runs; the upper levels fall below that and run on the 8-lane kernel"""
    rng = np.random.default_rng(arity)
    big, m_big = (4 ** 8 if arity == 4 else 2 ** 16) + 7, 3 * 2 ** 16 + 5
    sizes = rng.integers(0, 30, 301).tolist()
    adds = rng.integers(0, 4, 301).tolist()
    sizes[150], adds[150] = big, m_big
    la = 2 if arity == 4 else 1
    bound = lambda l: (sum(adds) >> (l * la)) + 2 * 301  # noqa: E731 (the host's bound of level l)
    assert bound(1) > 8192 and bound(3 if arity == 4 else 5) <= 8192
    flat = oracle_mod.fill_random(0xF20 + arity, sum(sizes))
    add = oracle_mod.fill_random(0xF30 + arity, sum(adds))
    old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), big)
    st = Dev(gpu_ctx, arity, 301, big + m_big)
    st.extract(old)
    bad, hashed = _counters()
    st.append(_torch(add), _torch(TS.offsets(adds)), bad, hashed)
    trees = [np.concatenate(p) for p in zip(_split(flat, sizes), _split(add, adds))]
    _same(st, _want(oracle_mod, arity, trees, big + m_big))
    assert int(bad) == 0 and int(hashed) == sum(FF.n_hashed(n, m, arity) for n, m in zip(sizes, adds))


# ---- 3. streaming ----
@pytest.mark.parametrize("arity", [4, 2])
def test_one_tree_streamed_in_chunks_from_an_empty_state(gpu_ctx, oracle_mod, arity):
    """5,000 leaves in chunks of 1, 3, 4, 17, 1,000 and the rest: after every chunk the root is the single-tree build's of the prefix"""
    import torch
    total = 5000
    flat = oracle_mod.fill_random(0xF40 + arity, total)
    d = _torch(flat)
    st = Dev(gpu_ctx, arity, 1, total)
    root = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    at, hashed_want = 0, 0
    bad, hashed = _counters()
    for chunk in (1, 3, 4, 17, 1000, total - 1025):
        st.append(d[at:at + chunk], _torch(np.array([0, chunk], dtype=np.uint64)), bad, hashed)
        hashed_want += FF.n_hashed(at, chunk, arity)
        at += chunk
        tree_device(gpu_ctx, arity, _tag(arity), d, at, root, None)
        torch.cuda.synchronize()
        assert torch.equal(st.roots[0], root) and int(st.counts[0]) == at, at
    assert at == total and int(bad) == 0 and int(hashed) == hashed_want
    _same(st, _want(oracle_mod, arity, [flat], total))


# ---- 4. agreement with the stored path ----
@pytest.mark.parametrize("arity", [4, 2])
def test_same_roots_as_the_stored_append_and_the_extraction_of_its_forest(gpu_ctx, oracle_mod, arity):
    import torch
    rng = np.random.default_rng(10 + arity)
    sizes = rng.integers(0, 300, 60).tolist() + [1, 4, 16, 64, 256, 2, 8, 32, 128]
    adds = rng.integers(0, 80, len(sizes)).tolist()
    adds[3], adds[-1] = 0, 0
    T, max_old, max_new = len(sizes), 300, 400
    flat = oracle_mod.fill_random(0xF50 + arity, sum(sizes))
    add = oracle_mod.fill_random(0xF60 + arity, sum(adds))
    old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), max_old)
    d_add, d_aoff = _torch(add), _torch(TS.offsets(adds))
    out = _outputs(arity, flat.shape[0] + add.shape[0], T, max_new)
    _stored_append(gpu_ctx, old, d_add, d_aoff, T, max_new, out)
    st = Dev(gpu_ctx, arity, T, max_new)
    st.extract(old)
    st.append(d_add, d_aoff)
    torch.cuda.synchronize()
    assert torch.equal(st.roots, out[3][:T])
    again = Dev(gpu_ctx, arity, T, max_new)
    again.extract(Grown(arity, out, T, max_new))
    _same(st, again.numpy(), "against the extraction of the stored append's forest")
    _same(st, _want(oracle_mod, arity, [np.concatenate(p) for p in zip(_split(flat, sizes), _split(add, adds))], max_new))


# ---- 5. refusals ----
@pytest.mark.parametrize("arity", [4, 2])
def test_refused_appends_leave_their_trees_untouched_and_are_counted(gpu_ctx, oracle_mod, arity):
    """one tree per rule among good trees: decreasing offsets (1, 6), n + m > max_leaves (3), a count above max_leaves (4: a corrupt
    state, with junk rows that must stay), the sum rule (7: its range overlaps tree 5's behind the decrease), a range past n_add (8)"""
    import torch
    max_leaves, n_add = 35, 40
    sizes = [10, 20, 7, 30, 3, 5, 9, 8, 12]
    aoff = np.array([0, 4, 2, 6, 12, 14, 40, 12, 38, 45], dtype=np.uint64)
    flat, add = oracle_mod.fill_random(0xF80 + arity, sum(sizes)), oracle_mod.fill_random(0xF90 + arity, n_add)
    st = Dev(gpu_ctx, arity, len(sizes), max_leaves)
    st.append(_torch(flat), _torch(TS.offsets(sizes)))  # from the empty state
    st.counts[4] = max_leaves + 5
    st.frontier[4] = 0x0123456789ABCDEF
    counts = list(sizes)
    counts[4] = max_leaves + 5
    m, refused = FF.accepted_appends(counts, aoff, n_add, max_leaves)
    assert m == [4, 0, 4, 0, 0, 26, 0, 0, 0] and refused == [False, True, False, True, True, False, True, True, True]
    before = st.numpy()
    bad, hashed = _counters()
    st.append(_torch(add), _torch(aoff), bad, hashed)
    after = st.numpy()
    assert int(bad) == 6 and int(hashed) == sum(FF.n_hashed(n, k, arity) for n, k in zip(sizes, m))
    trees = _split(flat, sizes)
    for t in range(len(sizes)):
        if refused[t]:
            assert all(np.array_equal(a[t], b[t]) for a, b in zip(after, before)), t
        else:
            grown = np.concatenate([trees[t], add[int(aoff[t]):int(aoff[t]) + m[t]]])
            rows, root = _want_one(oracle_mod, arity, grown, max_leaves)
            assert after[0][t] == grown.shape[0] and np.array_equal(after[1][t], rows) and np.array_equal(after[2][t], root), t
    # nothing to append at all: the refusals are still counted, nothing changes
    bad.zero_()
    st.append(None, _torch(np.array([0, 0, 0, 0, 0, 0, 0, 1, 0, 0], dtype=np.uint64)), bad, None)
    assert int(bad) == 3 and all(np.array_equal(a, b) for a, b in zip(st.numpy(), after))  # tree 4; past n_add = 0 (6); decreasing (7)
    torch.cuda.synchronize()


# ---- 6. edge values ----
@pytest.mark.parametrize("arity", [4, 2])
def test_unreduced_leaves_hash_as_their_residues_and_keep_their_bytes(gpu_ctx, oracle_mod, arity):
    """leaves with limbs >= p, up to 2^256 - 1: the roots and the rows above the leaves are the oracle's on the values mod p; row 0
    holds the leaves as they were given; a lone leaf's root is reduced"""
    sizes, adds = [0, 0, 3, 5, 16, 17, 0, 64], [1, 5, 2, 12, 1, 47, 4, 3]
    raw0, red0 = E.edge_scalars(0xFA0 + arity, sum(sizes))
    raw1, red1 = E.edge_scalars(0xFB0 + arity, sum(adds))
    raw1[0], red1[0] = E.limbs((1 << 256) - 1), E.limbs(((1 << 256) - 1) % E.P)  # the lone leaf of tree 0: the largest word
    assert not E.is_reduced(raw0).all() and not E.is_reduced(raw1[1:]).all()
    st = Dev(gpu_ctx, arity, len(sizes), 111)
    st.append(_torch(raw0), _torch(TS.offsets(sizes)))
    st.append(_torch(raw1), _torch(TS.offsets(adds)))
    counts, frontier, roots = st.numpy()
    stride = arity - 1
    for t, (r0, r1, x0, x1) in enumerate(zip(_split(raw0, sizes), _split(raw1, adds), _split(red0, sizes), _split(red1, adds))):
        raw, red = np.concatenate([r0, r1]), np.concatenate([x0, x1])
        rows, root = _want_one(oracle_mod, arity, red, 111)
        assert counts[t] == raw.shape[0] and np.array_equal(roots[t], E.reduce_mod_p(root)), t
        assert np.array_equal(frontier[t][stride:], rows[stride:]), t
        n = raw.shape[0]
        d = n % arity
        want0 = np.zeros((stride, 4), dtype=np.uint64)
        want0[:d] = raw[n - d:]
        assert np.array_equal(frontier[t][:stride], want0), t


# ---- 7. the scan over the trees, past one trip of its tile loop ----
@pytest.mark.parametrize("arity", [4, 2])
def test_more_trees_than_one_trip_of_the_scans_tile_loop(gpu_ctx, oracle_mod, arity):
    """BLOCK * SCAN_TILE trees fill one trip of scan_tile_row's loop; a few tiles more, every tree given 1 to 3 leaves, then one leaf
    appended to every 7th: a sample of 2,000 trees (both sides of the trip's edge among them) against the oracle, and the digest count"""
    T = BLOCK * SCAN_TILE + 2 * SCAN_TILE + 3
    rng = np.random.default_rng(arity)
    sizes = rng.integers(1, 4, T)
    adds = (np.arange(T) % 7 == 3).astype(np.int64)
    off, aoff = TS.offsets(sizes, dtype=np.int64), TS.offsets(adds, dtype=np.int64)
    flat, add = oracle_mod.fill_random(0xFC0 + arity, int(off[-1])), oracle_mod.fill_random(0xFD0 + arity, int(aoff[-1]))
    st = Dev(gpu_ctx, arity, T, 4)
    bad, hashed = _counters()
    st.append(_torch(flat), _torch(off.astype(np.uint64)), bad, hashed)
    first = int(hashed)
    st.append(_torch(add), _torch(aoff.astype(np.uint64)), bad, hashed)
    counts, frontier, roots = st.numpy()
    assert first == sum(int((sizes == n).sum()) * FF.n_hashed(0, n, arity) for n in (1, 2, 3))
    grown = sizes + adds
    want_second = sum(int(((adds == 1) & (sizes == n)).sum()) * FF.n_hashed(n, 1, arity) for n in (1, 2, 3))
    assert int(bad) == 0 and int(hashed) == first + want_second and np.array_equal(counts, grown)
    edge = BLOCK * SCAN_TILE
    sample = np.unique(np.concatenate([rng.integers(0, T, 1980), np.arange(edge - 8, edge + 8), [0, T - 1], np.arange(SCAN_TILE - 2, SCAN_TILE + 2)]))
    trees = [np.concatenate([flat[off[t]:off[t + 1]], add[aoff[t]:aoff[t + 1]]]) for t in sample]
    want = _want(oracle_mod, arity, trees, 4)
    assert np.array_equal(frontier[sample], want[1]) and np.array_equal(roots[sample], want[2])


# ---- 8. a side stream, twice in a row ----
@pytest.mark.parametrize("arity", [4, 2])
def test_two_appends_on_a_side_stream_without_a_host_sync(gpu_ctx, oracle_mod, arity):
    import torch
    rng = np.random.default_rng(20 + arity)
    T = 200
    x, y = rng.integers(0, 50, T).tolist(), rng.integers(0, 50, T).tolist()
    ax, ay = oracle_mod.fill_random(0xFE0 + arity, sum(x)), oracle_mod.fill_random(0xFF0 + arity, sum(y))
    d = [_torch(ax), _torch(TS.offsets(x)), _torch(ay), _torch(TS.offsets(y))]
    ref = Dev(gpu_ctx, arity, T, 100)
    ref.append(d[0], d[1])
    torch.cuda.synchronize()
    ref.append(d[2], d[3])
    torch.cuda.synchronize()
    st = Dev(gpu_ctx, arity, T, 100)
    bad, hashed = _counters()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st.append(d[0], d[1], bad, hashed)
        st.append(d[2], d[3], bad, hashed)
    torch.cuda.synchronize()
    _same(st, ref.numpy(), "side stream")
    assert int(bad) == 0 and int(hashed) == sum(FF.n_hashed(0, a, arity) + FF.n_hashed(a, b, arity) for a, b in zip(x, y))
    _same(st, _want(oracle_mod, arity, [np.concatenate(p) for p in zip(_split(ax, x), _split(ay, y))], 100))


# ---- 9. the module functions and the C++ mirror ----
def test_forest_frontier_holder_appends_and_extracts(gpu_ctx, oracle_mod):
    import torch
    from poseidon252_amd import merkle
    sizes, adds = [3, 1, 17, 0], [2, 0, 5, 4]
    flat, add = oracle_mod.fill_random(0xFE8, sum(sizes)), oracle_mod.fill_random(0xFE9, sum(adds))
    for arity in (4, 2):
        old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), 17)
        state, bad = merkle.ForestFrontier.from_forest(gpu_ctx, old.d, old.d_off, 4, 17, old.d_lv, old.roots, max_leaves=30, arity=arity)
        n_bad, n_hashed = state.append(_torch(add), _torch(TS.offsets(adds)))
        torch.cuda.synchronize()
        assert int(bad) == 1 and int(n_bad) == 0 and int(n_hashed) == sum(FF.n_hashed(n, m, arity) for n, m in zip(sizes, adds))
        want = _want(oracle_mod, arity, [np.concatenate(p) for p in zip(_split(flat, sizes), _split(add, adds))], 30)
        assert np.array_equal(_np(state.counts).astype(np.int64), want[0]) and np.array_equal(_np(state.frontier), want[1])
        assert np.array_equal(_np(state.roots), want[2])
        empty = merkle.ForestFrontier(gpu_ctx, 4, 30, arity)
        assert empty.frontier.shape == (4, FF.bound(30, arity), 4) and not bool(empty.roots.any())
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        merkle.ForestFrontier(gpu_ctx, 4, 30, 3)


def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_frontier_api", tmp_path))
