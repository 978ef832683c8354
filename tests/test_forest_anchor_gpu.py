"""Roots and openings of a grown forest against its EARLIER roots (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into;
csrc/forest_anchor.hip) on the GPU.  The references are the numpy model (testsupport/forestanchor.py, held to the oracle's truncated
rebuilds without a GPU), the only other route on the device — resize(keep = c) into a second forest, then the openings call — the oracle
itself for the edge values, and consistency extraction plus verification for the roots; never the call itself: every (tree, count,
leaf) of a small forest; every kind of bad input among valid neighbours; c == n_t and powers of the arity; edge-value leaves under
partial nodes; the launch geometry under both digest builds; the roots alone; one graph capture and replay; the C++ mirror and the
refusal program."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from testsupport import forestanchor as FA
from testsupport import forestfrontier as FF
from testsupport import treeshape as TS
from helpers import anchor_geometry_driver as GEO
from helpers.forest import Old, SENTINEL, _np, _tag, _torch, _tree
from helpers.percall import assert_rows_equal_golden, build_cpp_mirror, refusal_table, run_cpp_mirror

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
TAIL = 3
MAX_LEAVES = {4: 1024, 2: 128}  # the stride exceeds every depth


def sizes_of(arity):
    """trees of 1, 2, A, A + 1, A^2 - 1, A^2, A^2 + 1, 37 and (arity 4) 70 leaves"""
    a = arity
    return [1, 2, a, a + 1, a * a - 1, a * a, a * a + 1, 37] + ([70] if a == 4 else [])


def _call(ctx, arity, f, a_tree, a_count, o_anchor, o_leaf, openings=True):
    """one call on the built forest f (an Old) into canary-tailed buffers -> dict of numpy results; openings = False: k == 0 with the
    opening arrays NULL"""
    import torch
    m, k, D = len(a_tree), len(o_anchor) if openings else 0, TS.depth(f.max_leaves, arity)
    full = lambda shape, fill, dtype: torch.full(shape, fill, dtype=dtype, device="cuda:0")  # noqa: E731
    roots, depths = full((m + TAIL, 4), SENTINEL, torch.int64), full((m + TAIL,), CANARY, torch.uint8)
    bufs = [full((k + TAIL, 4), SENTINEL, torch.int64), full((k + TAIL, D, arity - 1, 4), SENTINEL, torch.int64), full((k + TAIL, D), CANARY, torch.uint8),
            full((k + TAIL,), CANARY, torch.uint8)]
    counters = torch.zeros(4, dtype=torch.int32, device="cuda:0")  # bad anchors, bad openings, and two words that must stay zero
    hashed = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    call = ctx.merkle4_forest_ragged_anchor_openings_device if arity == 4 else ctx.merkle2_forest_ragged_anchor_openings_device
    if openings:
        o_args = (_torch(np.asarray(o_anchor, np.uint32)), _torch(np.asarray(o_leaf, np.uint64)), k)
        o_bufs = (bufs[0][:k], bufs[1][:k] if D else None, bufs[2][:k] if D else None, bufs[3][:k])
    else:
        o_args, o_bufs = (None, None, 0), (None, None, None, None)
    call(_tag(arity), f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv if D else None, _torch(np.asarray(a_tree, np.uint32)), _torch(np.asarray(a_count, np.uint64)), m,
         *o_args, roots[:m], depths[:m], *o_bufs, counters[:1], counters[1:2], hashed[:1])
    torch.cuda.synchronize()
    intact = bool((roots[m:] == SENTINEL).all()) and bool((depths[m:] == CANARY).all()) and counters[2:].tolist() == [0, 0] and int(hashed[1]) == 0
    intact = intact and all(bool((b[k:] == fill).all()) for b, fill in zip(bufs, (SENTINEL, SENTINEL, CANARY, CANARY)))
    lv, sib, pos, dep = (_np(b[:k]) for b in bufs)
    return dict(roots=_np(roots[:m]), depths=depths[:m].cpu().numpy(), lv=lv, sib=sib, pos=pos, dep=dep, bad_anchors=int(counters[0]), bad=int(counters[1]),
                hashed=int(hashed[0]), intact=intact, D=D)


def _model(oracle_mod, arity, trees, built, a_tree, a_count, o_anchor, o_leaf, D):
    """the model's outputs for the same inputs: trees[t] = the tree's leaves or None for a bad / unknown tree, built[t] = (root, levels) of
    the oracle's build of the GROWN tree -> dict as _call returns"""
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    m, k = len(a_tree), len(o_anchor)
    roots, depths = np.zeros((m, 4), dtype=np.uint64), np.full(m, 0xFF, dtype=np.uint8)
    partial, hashed, bad_anchors = {}, 0, 0
    for a, (t, c) in enumerate(zip(a_tree, a_count)):
        leaves = trees[t] if t < len(trees) else None
        if leaves is None or not 1 <= c <= leaves.shape[0]:
            bad_anchors += 1
            continue
        n = leaves.shape[0]
        partial[a], h = FA.partial_nodes(leaves, built[t][1], n, int(c), arity, digest)
        hashed += h
        roots[a] = FA.root_of(leaves, built[t][1], n, int(c), arity, digest, partial=partial[a])
        depths[a] = TS.depth(int(c), arity)
    ws = []
    for a, i in zip(o_anchor, o_leaf):
        if a in partial:
            t, c = a_tree[a], int(a_count[a])
            ws.append(FA.opening_of(trees[t], built[t][1], trees[t].shape[0], c, int(i), arity, D, digest, partial=partial[a])[0])
        else:
            ws.append(FA.FW.Witness(arity, D))
    return dict(roots=roots, depths=depths, lv=np.array([w.leaf for w in ws]).reshape(k, 4), sib=np.array([w.siblings for w in ws]).reshape(k, D, arity - 1, 4),
                pos=np.array([w.positions for w in ws]).reshape(k, D), dep=np.array([w.depth for w in ws], dtype=np.uint8), bad_anchors=bad_anchors,
                bad=sum(w.bad() for w in ws), hashed=hashed)


def _same(got, want, what, names=("roots", "depths", "lv", "sib", "pos", "dep", "bad_anchors", "bad", "hashed")):
    for name in names:
        assert np.array_equal(got[name], want[name]), (what, name)


# ---- 1. every (tree, count, leaf) of a small forest ----
@pytest.fixture(scope="module", params=[4, 2])
def small(request, gpu_ctx, oracle_mod):
    """the trees of sizes_of(arity) and an empty (bad) tree in one forest; every (t, c) with 1 <= c <= n_t as an anchor, every i < c as
    an opening, shuffled; the call run once here"""
    arity = request.param
    sizes = sizes_of(arity) + [0]
    trees = [oracle_mod.fill_random(0xA80 + 16 * arity + t, n) if n else None for t, n in enumerate(sizes)]
    built = [_tree(oracle_mod, arity)(_tag(arity), x, want_levels=True)[:2] if x is not None else None for x in trees]
    f = Old(gpu_ctx, arity, np.concatenate([x for x in trees if x is not None]), TS.offsets(sizes), MAX_LEAVES[arity])
    pairs = [(t, c) for t, n in enumerate(sizes) for c in range(1, n + 1)]
    rng = np.random.default_rng(arity)
    pairs = [pairs[j] for j in rng.permutation(len(pairs))]
    a_tree, a_count = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    o_anchor = np.repeat(np.arange(len(pairs)), a_count)
    o_leaf = np.concatenate([np.arange(c) for c in a_count])
    order = rng.permutation(o_anchor.size)
    o_anchor, o_leaf = o_anchor[order], o_leaf[order]
    got = _call(gpu_ctx, arity, f, a_tree, a_count, o_anchor, o_leaf)
    return dict(arity=arity, sizes=sizes, trees=trees, built=built, f=f, a_tree=a_tree, a_count=a_count, o_anchor=o_anchor, o_leaf=o_leaf, got=got)


def test_every_anchor_and_opening_of_a_small_forest_equals_the_model(gpu_ctx, oracle_mod, small):
    """roots, depths, all four opening arrays and the digest count byte for byte the model's; the roots the oracle's builds of the first c
    leaves; canaries; nothing bad; every opening verifies against its anchor's root through the forest's own verify call"""
    import torch
    s, arity, got = small, small["arity"], small["got"]
    m, k = len(s["a_tree"]), len(s["o_anchor"])
    assert m == sum(s["sizes"]) and k == sum(n * (n + 1) // 2 for n in s["sizes"]) and k > (3000 if arity == 4 else 700)
    want = _model(oracle_mod, arity, s["trees"], s["built"], s["a_tree"], s["a_count"], s["o_anchor"], s["o_leaf"], got["D"])
    _same(got, want, "small forest")
    assert got["intact"] and got["bad_anchors"] == 0 and got["bad"] == 0
    assert got["hashed"] == sum(FA.old_digests(int(c), arity) for c in s["a_count"])
    for a in range(0, m, 7):  # the oracle's own truncated rebuild
        t, c = s["a_tree"][a], int(s["a_count"][a])
        rebuilt = FF.reduce_leaf(s["trees"][t][0]) if c == 1 else _tree(oracle_mod, arity)(_tag(arity), s["trees"][t][:c])[0]
        assert np.array_equal(got["roots"][a], rebuilt), (t, c)
    ok = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.merkle_forest_ragged_verify_device(_tag(arity), _torch(got["lv"]), _torch(got["sib"]), _torch(got["pos"]), _torch(got["dep"]), got["D"],
                                               _torch(s["o_anchor"].astype(np.uint32)), _torch(got["roots"]), m, ok, k, arity=arity)
    back = torch.zeros((k, 4), dtype=torch.int64, device="cuda:0")
    gpu_ctx.merkle_path_ragged_device(_tag(arity), _torch(got["lv"]), _torch(got["sib"]), _torch(got["pos"]), _torch(got["dep"]), got["D"], back, k, arity=arity)
    torch.cuda.synchronize()
    assert bool(ok.all()) and np.array_equal(_np(back), got["roots"][s["o_anchor"]])


def test_the_same_bytes_as_resize_then_openings(gpu_ctx, small):
    """the only other route: the forest cut to one count per tree by forest_ragged_resize (keep = c), then the plain openings call on the
    copy — for the counts 1, A, A^2 - 1, A^2, n_t - 1 and n_t of every tree that has them"""
    import torch
    from poseidon252_amd import merkle
    s, arity, got, f = small, small["arity"], small["got"], small["f"]
    A, T = arity, len(s["sizes"])
    anchor_of = {(int(t), int(c)): a for a, (t, c) in enumerate(zip(s["a_tree"], s["a_count"]))}
    by_anchor = {}
    for j, a in enumerate(s["o_anchor"]):
        by_anchor.setdefault(int(a), []).append(j)
    n_compared = 0
    for pick in (lambda n: 1, lambda n: A, lambda n: A * A - 1, lambda n: A * A, lambda n: n - 1, lambda n: n):
        keep = np.array([pick(n) if n and 1 <= pick(n) <= n else -1 for n in s["sizes"]], dtype=np.int64)  # (-1: the tree whole, not compared)
        c_leaves, c_off, c_lv, c_roots, _, _ = merkle.forest_ragged_resize(gpu_ctx, _tag(arity), f.d, f.d_off, T, f.max_leaves, f.d_lv, _torch(keep),
                                                                           max_leaves_new=f.max_leaves, arity=arity)
        trees = [t for t in range(T) if keep[t] > 0]
        rows = np.concatenate([by_anchor[anchor_of[(t, int(keep[t]))]] for t in trees])
        tid = s["a_tree"][s["o_anchor"][rows]]
        lv, sib, pos, dep, D = gpu_ctx.merkle_forest_ragged_openings_device(c_leaves, c_off, T, f.max_leaves, c_lv, _torch(tid.astype(np.uint32)),
                                                                            _torch(s["o_leaf"][rows].astype(np.uint64)), len(rows), arity=arity)
        torch.cuda.synchronize()
        assert D == got["D"]
        for name, o in zip(("lv", "sib", "pos", "dep"), (lv, sib, pos, dep)):
            assert np.array_equal(got[name][rows], _np(o)), (name, keep.tolist())
        for t in trees:
            assert np.array_equal(got["roots"][anchor_of[(t, int(keep[t]))]], _np(c_roots)[t]), (t, keep[t])
        n_compared += len(rows)
    assert n_compared > (400 if arity == 4 else 100)


# ---- 2. bad inputs, all in one call with valid neighbours ----
@pytest.mark.parametrize("arity", [4, 2])
def test_bad_anchors_and_openings_among_valid_neighbours(gpu_ctx, oracle_mod, arity):
    sizes = [5, 0, 17]
    trees = [oracle_mod.fill_random(0xAB0 + 16 * arity + t, n) if n else None for t, n in enumerate(sizes)]
    built = [_tree(oracle_mod, arity)(_tag(arity), x, want_levels=True)[:2] if x is not None else None for x in trees]
    f = Old(gpu_ctx, arity, np.concatenate([x for x in trees if x is not None]), TS.offsets(sizes), 64)
    #          valid   id >= n_trees  a bad tree  c == 0  c == n_t + 1  valid    id = 2^32 - 1   valid
    a_tree = [0,      3,             1,          2,      2,            2,       2 ** 32 - 1,    2]
    a_count = [3,     1,             1,          0,      18,           9,       1,              17]
    m = len(a_tree)
    #           valid  anchor id >= m  leaf == c  leaf >= n_t  under bad anchors   valid    valid (last leaf)  anchor id 2^32 - 1
    o_anchor = [0,     m,              0,         5,           1, 2, 3, 4, 6,      5,       7,                 2 ** 32 - 1]
    o_leaf = [1,       0,              3,         20,          0, 0, 0, 0, 0,      8,       16,                0]
    got = _call(gpu_ctx, arity, f, a_tree, a_count, o_anchor, o_leaf)
    want = _model(oracle_mod, arity, trees, built, a_tree, a_count, o_anchor, o_leaf, got["D"])
    _same(got, want, "bad inputs")
    assert got["intact"] and got["bad_anchors"] == 5 and got["bad"] == 9
    good_a, good_o = [0, 5, 7], [0, 9, 10]
    assert [d != 0xFF for d in got["depths"]] == [a in good_a for a in range(m)] and [d != 0xFF for d in got["dep"]] == [i in good_o for i in range(len(o_anchor))]
    for a in set(range(m)) - set(good_a):
        assert not got["roots"][a].any()
    for i in set(range(len(o_anchor))) - set(good_o):
        assert not got["lv"][i].any() and not got["sib"][i].any() and not got["pos"][i].any()
    assert got["hashed"] == sum(FA.old_digests(c, arity) for c in (3, 9, 17))
    for a in good_a:  # the neighbours: the oracle's rebuilds
        t, c = a_tree[a], a_count[a]
        assert np.array_equal(got["roots"][a], _tree(oracle_mod, arity)(_tag(arity), trees[t][:c])[0]), a
    # no anchor at all: every opening is bad, and nothing of the anchors is looked at
    none = _call(gpu_ctx, arity, f, [], [], [0, 1], [0, 0])
    assert none["intact"] and none["bad"] == 2 and none["bad_anchors"] == 0 and none["hashed"] == 0 and none["dep"].tolist() == [0xFF, 0xFF]
    assert not none["lv"].any() and not none["sib"].any() and not none["pos"].any()


# ---- 3. the whole tree, and the counts that hash nothing ----
@pytest.mark.parametrize("arity", [4, 2])
def test_the_whole_tree_is_the_plain_call_and_a_power_of_the_arity_hashes_nothing(gpu_ctx, oracle_mod, arity):
    import torch
    A = arity
    sizes = [A ** 3 + 5, 1, A ** 2, 37]
    flat = oracle_mod.fill_random(0xAC0 + arity, sum(sizes))
    off = TS.offsets(sizes, dtype=np.int64)
    f = Old(gpu_ctx, arity, flat, TS.offsets(sizes), max(sizes))
    T = len(sizes)
    # c == n_t of every tree, every leaf
    o_anchor = np.repeat(np.arange(T), sizes)
    o_leaf = np.concatenate([np.arange(n) for n in sizes])
    got = _call(gpu_ctx, arity, f, np.arange(T), sizes, o_anchor, o_leaf)
    lv, sib, pos, dep, D = gpu_ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, T, f.max_leaves, f.d_lv, _torch(o_anchor.astype(np.uint32)),
                                                                        _torch(o_leaf.astype(np.uint64)), len(o_leaf), arity=arity)
    torch.cuda.synchronize()
    assert got["intact"] and got["bad"] == 0 and got["bad_anchors"] == 0 and D == got["D"]
    for name, o in zip(("lv", "sib", "pos", "dep"), (lv, sib, pos, dep)):
        assert np.array_equal(got[name], _np(o)), name
    assert np.array_equal(got["roots"], _np(f.roots)) and got["hashed"] == sum(FA.old_digests(n, arity) for n in sizes)
    # c a power of the arity: the root is a stored node (c == 1: the leaf, reduced), and nothing is hashed
    a_tree, a_count = [0, 0, 0, 0, 1, 2, 2, 3, 3], [1, A, A ** 2, A ** 3, 1, A, A ** 2, 1, A ** 2]
    powers = _call(gpu_ctx, arity, f, a_tree, a_count, [0, 3, 3, 8], [0, 0, A ** 3 - 1, A ** 2 - 1])
    assert powers["intact"] and powers["hashed"] == 0 and powers["bad_anchors"] == 0 and powers["bad"] == 0
    for a, (t, c) in enumerate(zip(a_tree, a_count)):
        leaves = flat[off[t]:off[t] + c]
        assert np.array_equal(powers["roots"][a], FF.reduce_leaf(leaves[0]) if c == 1 else _tree(oracle_mod, arity)(_tag(arity), leaves)[0]), (t, c)
    assert powers["dep"].tolist() == [0, 3, 3, 2]


# ---- 4. edge values ----
@pytest.mark.parametrize("arity", [4, 2])
def test_edge_value_leaves_under_partial_nodes_and_as_a_sole_leaf(gpu_ctx, oracle_mod, arity):
    """0, 1, p - 1, p and 2^256 - 1 as the children of partial nodes (arity 4: P_1(3) = H(l0, l1, l2, 0); arity 2: P_1(3) = H(l2, 0) and
    P_1(5) = H(l4, 0)) and as the sole leaf of a c == 1 anchor: the roots are the oracle's on the values mod p, the openings carry the
    leaves' own bytes and verify"""
    import torch
    P = oracle_mod.P
    edges = [0, 1, P - 1, P, 2 ** 256 - 1]
    n = 11
    trees = []
    for j in range(len(edges)):
        x = oracle_mod.fill_random(0xAD0 + 16 * arity + j, n)
        for q in range(5):
            x[q] = oracle_mod.int_to_limbs(edges[(j + q) % len(edges)])
        trees.append(x)
    reduced = [np.array([FF.reduce_leaf(l) for l in x]) for x in trees]
    f = Old(gpu_ctx, arity, np.concatenate(trees), TS.offsets([n] * len(trees)), n)
    counts = (1, 3, 5, 6, n)
    a_tree = np.repeat(np.arange(len(trees)), len(counts))
    a_count = np.tile(counts, len(trees))
    o_anchor = np.repeat(np.arange(len(a_tree)), a_count)
    o_leaf = np.concatenate([np.arange(c) for c in a_count])
    got = _call(gpu_ctx, arity, f, a_tree, a_count, o_anchor, o_leaf)
    assert got["intact"] and got["bad"] == 0 and got["bad_anchors"] == 0
    for a, (t, c) in enumerate(zip(a_tree, a_count)):
        want = reduced[t][0] if c == 1 else _tree(oracle_mod, arity)(_tag(arity), reduced[t][:c])[0]
        assert np.array_equal(got["roots"][a], want), (t, c)
    assert np.array_equal(got["lv"], np.concatenate(trees)[a_tree[o_anchor] * n + o_leaf])  # the bytes handed in, not their residues
    k = len(o_anchor)
    ok = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.merkle_forest_ragged_verify_device(_tag(arity), _torch(got["lv"]), _torch(got["sib"]), _torch(got["pos"]), _torch(got["dep"]), got["D"],
                                               _torch(o_anchor.astype(np.uint32)), _torch(got["roots"]), len(a_tree), ok, k, arity=arity)
    torch.cuda.synchronize()
    assert bool(ok.all())
    # and byte for byte the model over the raw leaves, with the oracle's digest on the children's residues
    built = [_tree(oracle_mod, arity)(_tag(arity), r, want_levels=True)[:2] for r in reduced]
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), np.array([FF.reduce_leaf(c) for c in kids.reshape(-1, 4)]).reshape(kids.shape), arity, 1)  # noqa: E731
    for j in range(0, k, 3):
        a = o_anchor[j]
        t, c = a_tree[a], int(a_count[a])
        w = FA.opening_of(trees[t], built[t][1], n, c, int(o_leaf[j]), arity, got["D"], digest)[0]
        assert np.array_equal(got["sib"][j], w.siblings) and np.array_equal(got["pos"][j], w.positions) and got["dep"][j] == w.depth, (t, c, o_leaf[j])


# ---- 5. the launch geometry, under both digest builds ----
def test_launch_geometry_on_the_lane_group_build(gpu_ctx):
    """m in {1, 7, 8, 9, 63, 64, 65, 257} and k in {1, 255, 256, 257, 5000} on one tree of A^5 + 3 leaves (helpers/anchor_geometry_driver.py):
    every opening verifies against the anchor roots, every root is the consistency route's, the digest count does not depend on k"""
    for arity in (4, 2):
        r = GEO.run(gpu_ctx, arity)
        assert r["calls"] == len(GEO.M) * len(GEO.K) and r["digests"] > 0


def test_launch_geometry_on_the_one_lane_build():
    """the same in a child under P252_COOP_MAX_NODES=0 (read once per process): the anchors' digests run the one-lane build"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "anchor_geometry_driver.py")], cwd=ROOT,
                       env=dict(os.environ, P252_COOP_MAX_NODES="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report["anchor_geometry"] == "ok" and report["coop_max_nodes"] == "0" and sorted(report["arities"]) == ["2", "4"]


# ---- 6. the roots alone ----
def test_the_roots_alone_with_null_opening_arrays(gpu_ctx, small):
    s, arity, got = small, small["arity"], small["got"]
    alone = _call(gpu_ctx, arity, s["f"], s["a_tree"], s["a_count"], [], [], openings=False)
    assert alone["intact"] and alone["bad_anchors"] == 0 and alone["bad"] == 0
    _same(alone, got, "roots alone", names=("roots", "depths", "hashed"))


# ---- 7. one capture, one replay ----
@pytest.mark.parametrize("arity", [4, 2])
def test_one_graph_capture_and_replay_gives_the_direct_calls_bytes(gpu_ctx, oracle_mod, arity):
    """the call is a linear chain of launches on the caller's stream: captured once its scratch is warm, replayed once"""
    import torch
    sizes = [70, 1, 37, 16]
    flat = oracle_mod.fill_random(0xAE0 + arity, sum(sizes))
    f = Old(gpu_ctx, arity, flat, TS.offsets(sizes), 128)
    rng = np.random.default_rng(0xAE + arity)
    a_tree = np.array([0, 0, 1, 2, 2, 3, 3, 5])
    a_count = np.array([70, 33, 1, 37, 22, 16, 9, 1])
    o_anchor = rng.integers(0, len(a_tree), 300)
    o_leaf = (rng.random(300) * np.maximum(a_count[o_anchor], 1)).astype(np.int64)
    direct = _call(gpu_ctx, arity, f, a_tree, a_count, o_anchor, o_leaf)
    assert direct["intact"] and direct["bad_anchors"] == 1 and direct["bad"] == int((o_anchor == 7).sum())
    m, k, D = len(a_tree), len(o_anchor), direct["D"]
    d_at, d_ac = _torch(a_tree.astype(np.uint32)), _torch(a_count.astype(np.uint64))
    d_oa, d_ol = _torch(o_anchor.astype(np.uint32)), _torch(o_leaf.astype(np.uint64))
    full = lambda shape, fill, dtype: torch.full(shape, fill, dtype=dtype, device="cuda:0")  # noqa: E731
    out = [full((m, 4), SENTINEL, torch.int64), full((m,), CANARY, torch.uint8), full((k, 4), SENTINEL, torch.int64), full((k, D, arity - 1, 4), SENTINEL, torch.int64),
           full((k, D), CANARY, torch.uint8), full((k,), CANARY, torch.uint8)]
    counters, hashed = torch.zeros(2, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0")
    method = gpu_ctx.merkle4_forest_ragged_anchor_openings_device if arity == 4 else gpu_ctx.merkle2_forest_ragged_anchor_openings_device
    call = lambda: method(_tag(arity), f.d, f.d_off, f.n_trees, f.max_leaves, f.d_lv, d_at, d_ac, m, d_oa, d_ol, k, *out, counters[:1], counters[1:], hashed)  # noqa: E731
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()  # warm-up: the stream's scratch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    out[0].fill_(SENTINEL), out[2].fill_(SENTINEL), out[3].fill_(SENTINEL)
    out[1].fill_(CANARY), out[4].fill_(CANARY), out[5].fill_(CANARY)
    counters.zero_(), hashed.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed = dict(zip(("roots", "depths", "lv", "sib", "pos", "dep"), (_np(t) if t.dtype == torch.int64 else t.cpu().numpy() for t in out)),
                    bad_anchors=int(counters[0]), bad=int(counters[1]), hashed=int(hashed))
    _same(replayed, direct, "replay")


def test_trivial_sizes(gpu_ctx, oracle_mod):
    """max_leaves == 1 has no rows and no levels: every anchor is a one-leaf tree at c == 1 or a bad one"""
    for arity in (4, 2):
        leaves = oracle_mod.fill_random(0xAF0 + arity, 3)
        f = Old(gpu_ctx, arity, leaves, np.array([0, 1, 2, 3], dtype=np.uint64), 1)
        got = _call(gpu_ctx, arity, f, [0, 2, 1, 3, 1], [1, 1, 2, 1, 0], [0, 1, 2, 0, 4], [0, 0, 0, 1, 0])
        assert got["D"] == 0 and got["intact"] and got["bad_anchors"] == 3 and got["bad"] == 3 and got["hashed"] == 0
        assert got["depths"].tolist() == [0, 0, 0xFF, 0xFF, 0xFF] and got["dep"].tolist() == [0, 0, 0xFF, 0xFF, 0xFF]
        assert np.array_equal(got["roots"][:2], _np(f.roots)[[0, 2]]) and not got["roots"][2:].any()
        assert np.array_equal(got["lv"][:2], leaves[[0, 2]]) and not got["lv"][2:].any()


# ---- 8. the mirrors ----
def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_anchor_api", tmp_path))


def test_refusal_program_on_gpu(gpu_ctx, tmp_path):
    assert_rows_equal_golden(refusal_table("anchor_refusal_table", tmp_path), "anchor_refusals")
