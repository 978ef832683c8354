"""The shapes of tests/scanwidth.py meet the conditions they are here for — every two-level scan makes three trips (a carry set on one
trip and added to on the next) with real elements behind every trip border — asserted on the numpy models of testsupport/ alone, no GPU;
and scanwidth's own vectorised expectations are held to those models and to the oracle on forests small enough for them."""
import numpy as np
import pytest

import edgecases as E
import scanwidth as S
from testsupport.forestappend import forest_append_model, forest_resize_model, model_leaves
from testsupport.multiproofmodel import forest_multiproof_counts, forest_multiproof_extract, multiproof_model
from testsupport import treeshape as TS

SMALL = 5000


# ---------------------------------------------------------------------------------------------- the conditions
def check_tree_scans(n_trees, kernels=S.TREE_KERNELS):
    """three trips of every per-tree scan, the last trip's last tile partial -> {kernel: tiles}"""
    out = {}
    for k in kernels:
        tile, per_trip = S.SCANS[k]
        assert S.trips(k, n_trees) == 3 and S.tiles(k, n_trees) > 2 * per_trip + 1, (k, n_trees, S.tiles(k, n_trees))
        assert n_trees % tile, (k, "the last tile is whole")
        out[k] = S.tiles(k, n_trees)
    return out


def check_wide_forest(f):
    a, T = f.arity, f.sizes.size
    tiles = check_tree_scans(T)
    top = 2 * a + 1
    assert f.sizes.min() == 1 and f.sizes.max() == top == f.max_leaves and np.unique(f.sizes).size == top
    share = np.bincount(f.sizes, minlength=top + 1)[1:] / T
    assert (np.abs(share - 1 / top) < 0.01).all()  # shuffled evenly: many one-leaf trees, most trees with two levels
    assert (f.sizes > a).mean() > 0.5
    for t in S.at_trip_borders(T):
        assert TS.depth(int(f.sizes[t]), a) >= 2, t
    assert len(S.at_trip_borders(T)) == 4 and len(S.trip_borders(T)) == 12
    # one-leaf trees with limbs >= p on both sides of every trip border
    assert len(f.unreduced) >= 4 and (f.sizes[f.unreduced] == 1).all() and not E.is_reduced(f.flat[f.off[f.unreduced]]).any()
    for c in range(S.TREE_CHUNK, T, S.TREE_CHUNK):
        assert any(t < c for t in f.unreduced) and any(t >= c for t in f.unreduced)
    assert f.unreduced[-1] >= 2 * S.TREE_CHUNK
    # every other leaf is below p (the expectation digests them unreduced)
    other = np.ones(f.flat.shape[0], dtype=bool)
    other[f.off[f.unreduced]] = False
    assert int(f.flat[other].max()) < 1 << 60
    # the oracle's share is small, and holds the trees it is there for
    need = set(S.trip_borders(T)) | {0, T - 1} | set(f.unreduced)
    assert need <= set(f.oracle_ids) and len(f.oracle_ids) <= len(need) + 200
    return tiles


def check_single(arity, case, n, pos):
    """three trips of k_mp_scan_tiles at level 0, real elements behind the borders of the upper levels -> tiles per level"""
    proof_nodes, Sl, _ = multiproof_model(n, pos, arity)
    counts = [s.size for s in Sl]
    ch = S.chunk("k_mp_scan_tiles")
    assert counts[0] > 2 * ch and S.trips("k_mp_scan_tiles", counts[0]) >= 3, counts[0]
    length = sum(p.size for p in proof_nodes)
    assert length > 0
    if case == "dense":
        if arity == 4:
            assert counts[1] > ch, counts
        else:
            assert counts[1] > 2 * ch and counts[2] > ch, counts
    else:
        assert pos.size == 140000 and length > ch + 1  # (a proof node beyond offset `ch` exists to be flipped)
    return [S.tiles("k_mp_scan_tiles", c) for c in counts], length


# ---------------------------------------------------------------------------------------------- constants and trips
def test_constants_are_read_from_csrc():
    assert all(S.C[n] > 0 for n in S.NAMES)
    assert S.SCANS["k_fr_scan_tiles"][0] == S.C["FR_BLOCK"] * S.C["FR_ITEMS"] and S.SCANS["k_fa_scan_tiles"][0] == S.C["FOREST_APPEND_SCAN_TILE"]
    # the three per-tree scans share one tile and one trip today; if they part, the wide forest follows the largest and the
    # conditions below say which kernel no longer makes its three trips
    print("constants:", {n: S.C[n] for n in S.NAMES}, "wide forest:", S.WIDE_TREES, "trees; list chunk", S.LIST_CHUNK)
    assert S.WIDE_TREES == 2 * S.TREE_CHUNK + 3 * S.TREE_TILE + 5


@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_forest_meets_its_conditions(arity):
    f = S.wide_forest(arity)
    tiles = check_wide_forest(f)
    print("wide forest, arity %d: %d trees, %d leaves, tiles %s, %d trees for the oracle" % (arity, f.sizes.size, f.flat.shape[0], tiles, len(f.oracle_ids)))


def test_narrowed_shapes_fail_the_conditions():
    with pytest.raises(AssertionError):
        check_tree_scans(S.TREE_CHUNK)  # 524,288 trees: one trip
    with pytest.raises(AssertionError):
        check_tree_scans(2 * S.TREE_CHUNK + 1)  # a third trip of one tile: no whole tile behind the second border
    n = S.single_n(4)
    with pytest.raises(AssertionError):
        check_single(4, "sparse", n, S.sparse(n, k=S.LIST_CHUNK))  # 65,536 positions: one trip
    with pytest.raises(AssertionError):  # random positions alone: level 1 of the arity-4 tree stays inside one trip
        check_single(4, "dense", n, S.sparse(n, k=200000))


# ---------------------------------------------------------------------------------------------- the expectations, held to oracle and models
@pytest.mark.parametrize("arity", S.ARITIES)
def test_expected_forest_and_siblings_against_the_oracle(oracle_mod, arity):
    f = S.wide_forest(arity, SMALL)
    roots, levels, lo = S.expected_forest(f.sizes, f.off, f.flat, arity, S.oracle_digest(arity))
    built = S.oracle_trees(arity, f.sizes, f.off, f.flat, list(range(SMALL)))
    for t in range(SMALL):
        assert np.array_equal(roots[t], built[t][0]) and np.array_equal(levels[lo[t]:lo[t + 1]], built[t][1]), t
    assert E.is_reduced(roots).all() and lo[-1] == sum(sum(TS.level_widths(int(n), arity)) for n in f.sizes)
    rng = np.random.default_rng(arity)
    tid = np.sort(rng.choice(SMALL, 800, replace=False))
    lid = (rng.random(800) * f.sizes[tid]).astype(np.int64)
    D = TS.depth(f.max_leaves, arity)
    sib, pos, depths = S.expected_siblings(f.sizes, f.off, f.flat, lo, levels, tid, lid, arity, D)
    assert np.array_equal(depths, [TS.depth(int(n), arity) for n in f.sizes[tid]])
    raw = f.flat[f.off[tid] + lid]
    assert np.array_equal(E.rehash(E._mtag(arity), arity, E.reduce_mod_p(raw), sib, pos, depths), roots[tid])


@pytest.mark.parametrize("arity", S.ARITIES)
def test_resize_counts_and_leaves_against_the_models(arity):
    f = S.wide_forest(arity, SMALL)
    ap = S.wide_append(arity, SMALL)
    M = forest_append_model(f.off, f.flat.shape[0], f.max_leaves, ap["add_off"], ap["add"].shape[0], ap["max_new"], arity)
    n_new, hashed, bad = S.resize_counts(f.sizes, None, ap["m"], arity)
    assert not any(M["refused"]) and np.array_equal(n_new, M["n_new"]) and (hashed, bad) == (M["n_hashed"], M["n_bad"]) and hashed > 0
    flat2, off2 = S.resize_leaves(f.off, f.flat, f.sizes.tolist() + [0] * (ap["T_new"] - SMALL), ap["add_off"], ap["add"])
    assert np.array_equal(off2, M["offsets_new"]) and np.array_equal(flat2, model_leaves(M, f.flat, ap["add"]))
    rs = S.wide_resize(arity, n_new)
    M = forest_resize_model(off2, flat2.shape[0], ap["max_new"], rs["keep"], rs["add_off"], rs["add"].shape[0], rs["max_new"], arity)
    n3, hashed, bad = S.resize_counts(n_new, rs["keep"], rs["m"], arity)
    assert not any(M["refused"]) and np.array_equal(n3, M["n_new"]) and (hashed, bad) == (M["n_hashed"], M["n_bad"]) and bad == rs["to_zero"].size
    flat3, off3 = S.resize_leaves(off2, flat2, M["k"], rs["add_off"], rs["add"])
    assert np.array_equal(off3, M["offsets_new"]) and np.array_equal(flat3, model_leaves(M, flat2, rs["add"]))


@pytest.mark.parametrize("arity", S.ARITIES)
def test_wide_append_and_resize_meet_their_conditions(arity):
    f, ap = S.wide_forest(arity), S.wide_append(arity)
    T = f.sizes.size
    assert ap["T_new"] == T + S.TREE_TILE + 3 and check_tree_scans(ap["T_new"], ("k_fa_scan_tiles", "k_fr_scan_tiles"))
    m = ap["m"]
    assert 0.1 < (m[:T] > 0).mean() < 0.3 and m[:T].max() == 3 and (m[S.trip_borders(T)] > 0).all() and (m[T:] > 0).all()
    n_new, hashed, bad = S.resize_counts(f.sizes, None, m, arity)
    assert bad == 0 and int(n_new.max()) <= ap["max_new"]
    rs = S.wide_resize(arity, n_new)
    T2 = rs["T_new"]
    assert T2 == ap["T_new"] - S.TREE_TILE - 7 and check_tree_scans(T2, ("k_fa_scan_tiles", "k_fr_scan_tiles"))
    keep, m2 = rs["keep"], rs["m"]
    cut = keep < n_new[:T2].astype(np.uint64)
    assert 0.15 < cut.mean() < 0.35 and (keep[rs["to_one"]] <= 1).all() and (m2 > 0).any() and (cut & (m2 > 0)).any()
    b = S.trip_borders(T2)
    assert cut[b[0::2]].all() and (m2[b] > 0).all()
    n3, hashed2, bad2 = S.resize_counts(n_new, keep, m2, arity)
    assert bad2 == rs["to_zero"].size > 0 and int(n3.max()) <= rs["max_new"] and rs["to_zero"].max() > 2 * S.TREE_CHUNK
    # every DIRTY row has digests on all three trips
    for sizes, k_, m_ in ((f.sizes, None, m), (n_new, keep, m2)):
        for lo_, hi_ in ((0, S.TREE_CHUNK), (S.TREE_CHUNK, 2 * S.TREE_CHUNK), (2 * S.TREE_CHUNK, m_.size)):
            part = S.resize_counts(sizes[lo_:hi_], None if k_ is None else k_[lo_:hi_], m_[lo_:hi_], arity)
            assert part[1] > 0
    print("arity %d: append %d -> %d trees, %d digests; resize -> %d trees, %d digests, %d bad" % (arity, T, ap["T_new"], hashed, T2, hashed2, bad2))


@pytest.mark.parametrize("arity", S.ARITIES)
def test_forest_multiproof_fast_against_the_model(arity):
    f = S.wide_forest(arity, SMALL)
    sizes = f.sizes.copy()
    sizes[[7, 4000]] = [300, 1000]  # two deeper trees, many pairs in each
    off, lo = TS.offsets(sizes, dtype=np.int64), TS.block_starts(sizes, arity)
    flat, levels = S.leaves(off[-1], 1), S.leaves(lo[-1], 2)  # (extraction only copies: any bytes serve as levels)
    rng = np.random.default_rng(arity)
    tid, lid = S._small_pairs(sizes, np.nonzero(rng.random(SMALL) < 0.3)[0], rng)
    keep = ~np.isin(tid, [7, 4000])
    tid = np.concatenate([tid[keep], np.full(150, 7), np.full(700, 4000)])
    lid = np.concatenate([lid[keep], np.sort(rng.choice(300, 150, replace=False)), np.sort(rng.choice(1000, 700, replace=False))])
    order = np.lexsort((lid, tid))
    tid, lid = tid[order], lid[order]
    fast = S.forest_multiproof_fast(sizes, tid, lid, arity, off, flat, lo, levels)
    po, hashed = forest_multiproof_counts(sizes, tid, lid, arity)
    out, proof, po2 = forest_multiproof_extract(flat, off, levels, tid, lid, arity)
    assert np.array_equal(fast["po"], po) and np.array_equal(po, po2) and fast["hashed"] == hashed
    assert np.array_equal(fast["out"], out) and np.array_equal(fast["proof"], proof)
    counts_only = S.forest_multiproof_fast(sizes, tid, lid, arity)
    assert np.array_equal(counts_only["po"], po) and counts_only["counts"] == fast["counts"] and fast["counts"][0] == tid.size


# ---------------------------------------------------------------------------------------------- multiproof shapes
@pytest.mark.parametrize("case", ["dense", "sparse"])
@pytest.mark.parametrize("arity", S.ARITIES)
def test_single_tree_positions_meet_their_conditions(arity, case):
    n = S.single_n(arity)
    assert n == (4 ** 9 + 1 if arity == 4 else 2 ** 18 + 1)
    pos = S.single_positions(arity, case)
    if case == "dense":
        assert 0.97 * n < pos.size < 0.99 * n and pos[-1] == n - 1
    tiles, length = check_single(arity, case, n, pos)
    print("single tree, arity %d, %s: k %d, proof %d scalars, tiles per level %s" % (arity, case, pos.size, length, tiles))


def _fm_counts(c):
    r = S.forest_multiproof_fast(c.sizes, c.tid, c.lid, c.arity)
    return r, [S.tiles("k_fm_scan_tiles", n) for n in r["counts"]]


@pytest.mark.parametrize("arity", S.ARITIES)
def test_forest_multiproof_wide_meets_its_conditions(arity):
    c = S.fm_wide(arity)
    T, ch = c.sizes.size, S.chunk("k_fm_scan_tiles")
    r, tiles = _fm_counts(c)
    per_tree = np.bincount(c.tid, minlength=T)
    assert c.tid.size >= 4 * ch and S.trips("k_fm_scan_tiles", c.tid.size) >= 4
    assert 0.2 < (per_tree > 0).mean() < 0.3 and per_tree.max() <= 2  # every tree a segment of its own, shorter than a tile
    assert S.trips("k_fm_tree_scan", T) == 3 and (per_tree[S.trip_borders(T)] > 0).all()
    assert r["counts"][1] > 2 * ch  # level 1 makes three trips as well
    first = S.first_pair_index(c)
    assert first[c.victim] > 2 * ch
    # proof scalars on every trip of the tree scan
    lens = np.diff(r["po"].astype(np.int64))
    assert all(lens[lo_:hi_].sum() > 0 for lo_, hi_ in ((0, S.TREE_CHUNK), (S.TREE_CHUNK, 2 * S.TREE_CHUNK), (2 * S.TREE_CHUNK, T)))
    print("forest multiproof wide, arity %d: %d pairs in %d trees, proof %d scalars, tiles per level %s, tree tiles %d"
          % (arity, c.tid.size, int((per_tree > 0).sum()), int(r["po"][-1]), tiles, S.tiles("k_fm_tree_scan", T)))


@pytest.mark.parametrize("arity", S.ARITIES)
def test_forest_multiproof_long_run_meets_its_conditions(arity):
    c = S.fm_long_run(arity)
    ch = S.chunk("k_fm_scan_tiles")
    assert c.big == 3 and c.sizes[3] == S.single_n(arity) and (c.sizes[:3] < 10).all() and (c.sizes[4:] < 10).all() and c.sizes.size > 5
    first = S.first_pair_index(c)
    lo_, hi_ = first[3], first[4]  # the big tree's run of the pair list
    whole = hi_ // ch - (lo_ // ch + 1)  # whole chunks inside the run, none of them starting at the tree's start
    assert lo_ > 0 and whole >= 2, (lo_, hi_)
    assert first[c.victim] > 2 * ch
    r, tiles = _fm_counts(c)
    po, hashed = forest_multiproof_counts(c.sizes, c.tid, c.lid, arity)
    assert np.array_equal(r["po"], po) and r["hashed"] == hashed
    print("forest multiproof long run, arity %d: %d pairs, the big tree's run %d .. %d, tiles per level %s" % (arity, c.tid.size, lo_, hi_, tiles))


@pytest.mark.parametrize("arity", S.ARITIES)
def test_forest_multiproof_aligned_meets_its_conditions(arity):
    ch = S.chunk("k_fm_scan_tiles")
    for shift in (0, 1, 2):
        c = S.fm_aligned(arity, shift)
        first = S.first_pair_index(c)
        assert first[1] == ch - 1 + shift and first[c.victim] > 2 * ch and sorted(first) == [0, 1, 2, 3, 4]
        r, tiles = _fm_counts(c)
        po, hashed = forest_multiproof_counts(c.sizes, c.tid, c.lid, arity)
        assert np.array_equal(r["po"], po) and r["hashed"] == hashed and int(po[2] - po[1]) > 0
        print("forest multiproof aligned, arity %d: tree 1 starts at element %d, tiles per level %s" % (arity, first[1], tiles))


# ---------------------------------------------------------------------------------------------- the ragged hash
def _bucket(length):
    """bucket_of of csrc/ragged.hip"""
    b, exact, sub = S.blocks_of(length), S.C["RAGGED_EXACT_BLOCKS"], S.C["RAGGED_SUB_LOG2"]
    if b < exact:
        return b
    k = b.bit_length() - 1
    return exact + (k - 10) * (1 << sub) + ((b >> (k - sub)) & ((1 << sub) - 1))


def test_ragged_batches_reach_the_octave_buckets():
    exact = S.C["RAGGED_EXACT_BLOCKS"]
    assert exact == 1 << 10  # (bucket_of's octave arithmetic starts at 2^10)
    assert S.RAGGED_MAX_LEN == 8 * exact + 1 and len(S.RAGGED_LONG) == 12 and max(S.RAGGED_LONG) == S.RAGGED_MAX_LEN
    assert sorted(set(S.RAGGED_LONG)) == [4091, 4092, 4093, 4096, 4097, 6000, 8188, 8189, 8192, 8193]
    buckets = sorted({_bucket(n) for n in S.RAGGED_LONG})
    assert buckets[0] == exact - 1 and buckets[1] == exact  # the last exact bucket, the first octave bucket
    assert _bucket(4092) == exact - 1 and _bucket(4093) == exact and _bucket(8188) + 1 == _bucket(8189) == _bucket(8193)
    assert len(buckets) >= 5 and buckets[-1] < S.C["RAGGED_EXACT_BLOCKS"] + 53 * 16
    assert S.RAGGED_SIZES == (9000, 100)  # past the lane-group switch (8,192 messages), and inside it
    for n in S.RAGGED_SIZES:
        flat, off, lens = S.ragged_batch(n)
        long = lens > 42
        assert sorted(lens[long].tolist()) == sorted(S.RAGGED_LONG) and lens.min() >= 1 and int(off[-1]) == flat.shape[0]
