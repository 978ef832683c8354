"""The openings of marked leaves kept current across appends to a forest kept only as its frontiers
(p252_merkle{4,2}_forest_frontier_append_witness_device_into; csrc/forest_witness.hip) on the GPU.  The references are the openings
call on a fresh stored build of ALL leaves every tree was given so far, and the numpy model (testsupport/forestwitness.py, checked
against the oracle without a GPU) — never the call itself: a witness for every leaf of a forest of every small transition, the bad and
stale ones among them; one set of witnesses carried through six appends; one larger tree whose computed runs span several blocks; the
trivial sizes; the Python holders and the C++ mirror."""
import numpy as np
import pytest

from testsupport import forestfrontier as FF
from testsupport import forestwitness as FW
from testsupport import treeshape as TS
from helpers.forest import Old, SENTINEL, _np, _tag, _torch, _tree
from helpers.percall import build_cpp_mirror, run_cpp_mirror

pytestmark = pytest.mark.gpu

CANARY = 0xA5


class Wits:
    """k witnesses on the device at the stride D >= 1, every array with a canary tail behind the k entries the call is given"""

    def __init__(self, arity, D, tid, lid, tail=3):
        import torch
        self.arity, self.D, self.k = arity, D, len(tid)
        k = self.k
        self.tid, self.lid = _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64))
        self.all = [torch.full((k + tail, 4), SENTINEL, dtype=torch.int64, device="cuda:0"),
                    torch.full((k + tail, D, arity - 1, 4), SENTINEL, dtype=torch.int64, device="cuda:0"),
                    torch.full((k + tail, D), CANARY, dtype=torch.uint8, device="cuda:0"),
                    torch.full((k + tail,), CANARY, dtype=torch.uint8, device="cuda:0")]
        self.leaves, self.sib, self.pos, self.dep = (a[:k] for a in self.all)

    def put(self, arrays):
        for mine, a in zip((self.leaves, self.sib, self.pos, self.dep), arrays):
            mine.copy_(_torch(np.ascontiguousarray(a)).reshape(mine.shape))

    def get(self):
        import torch
        torch.cuda.synchronize()
        return [_np(a) for a in (self.leaves, self.sib, self.pos, self.dep)]

    def canaries_intact(self):
        k = self.k
        return all(bool((a[k:] == fill).all()) for a, fill in zip(self.all, (SENTINEL, SENTINEL, CANARY, CANARY)))

    def append(self, ctx, state, d_add, d_aoff, bad=None, hashed=None, bad_witness=None):
        call = ctx.merkle4_forest_frontier_append_witness_device if self.arity == 4 else ctx.merkle2_forest_frontier_append_witness_device
        call(_tag(self.arity), state.counts, state.frontier, state.roots, state.n_trees, state.max_leaves, d_add, d_aoff, self.tid, self.lid, self.k,
             self.leaves, self.sib, self.pos, self.dep, bad, hashed, bad_witness)

    def verify(self, ctx, state):
        import torch
        ok = torch.full((self.k,), 7, dtype=torch.uint8, device="cuda:0")
        ctx.merkle_forest_ragged_verify_device(_tag(self.arity), self.leaves, self.sib, self.pos, self.dep, self.D, self.tid, state.roots, state.n_trees,
                                               ok, self.k, arity=self.arity)
        torch.cuda.synchronize()
        return ok.cpu().numpy()


def _counters():
    import torch
    return (torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0"),
            torch.zeros(1, dtype=torch.int32, device="cuda:0"))


def _state_of(ctx, arity, trees, max_leaves):
    """the ForestFrontier of the stored forest of these trees (lists of (n, 4) leaves; an empty tree is an empty one), and that forest"""
    import torch
    from poseidon252_amd import merkle
    sizes = [t.shape[0] for t in trees]
    old = Old(ctx, arity, np.concatenate(trees), TS.offsets(sizes), max_leaves)
    state, _ = merkle.ForestFrontier.from_forest(ctx, old.d, old.d_off, len(trees), max_leaves, old.d_lv, old.roots, arity=arity)
    torch.cuda.synchronize()
    return state, old


def _stored_openings(ctx, arity, old, tid, lid):
    """[leaves, siblings, positions, depths] (numpy) of the pairs out of a stored forest, at the stride of its max_leaves"""
    import torch
    lv, sib, pos, dep, _ = ctx.merkle_forest_ragged_openings_device(old.d, old.d_off, old.n_trees, old.max_leaves, old.d_lv,
                                                                    _torch(np.asarray(tid, np.uint32)), _torch(np.asarray(lid, np.uint64)), len(tid),
                                                                    arity=arity)
    torch.cuda.synchronize()
    return [_np(lv), _np(sib), _np(pos), _np(dep)]


def _copy_state(state):
    from poseidon252_amd import merkle
    return merkle.ForestFrontier(state.ctx, state.n_trees, state.max_leaves, state.arity, counts=state.counts.clone(), frontier=state.frontier.clone(),
                                 roots=state.roots.clone())


def _plain(ctx, state, d_add, d_aoff):
    bad, hashed, _ = _counters()
    call = ctx.merkle4_forest_frontier_append_device if state.arity == 4 else ctx.merkle2_forest_frontier_append_device
    call(_tag(state.arity), state.counts, state.frontier, state.roots, state.n_trees, state.max_leaves, d_add, d_aoff, bad, hashed)
    return bad, hashed


def _same_state(a, b):
    import torch
    torch.cuda.synchronize()
    return torch.equal(a.counts, b.counts) and torch.equal(a.frontier, b.frontier) and torch.equal(a.roots, b.roots)


def _differ(got, want):
    """indices of the witnesses whose four arrays are not all equal"""
    k = got[3].shape[0]
    bad = np.zeros(k, bool)
    for g, w in zip(got, want):
        bad |= (np.asarray(g).reshape(k, -1) != np.asarray(w).reshape(k, -1)).any(axis=1)
    return np.nonzero(bad)[0]


def _model(oracle_mod, arity, D, max_leaves, before, grow, tid, lid, seeded):
    """the model's witnesses after tree t of `before` received grow[t], from the arrays `seeded`; an unknown tree: bad"""
    digest = lambda kids: oracle_mod.hash_batch(_tag(arity), kids, arity, 1)  # noqa: E731
    states, computed = [], []
    for old, add in zip(before, grow):
        n = old.shape[0]
        if n:
            root, levels = _tree(oracle_mod, arity)(_tag(arity), old, want_levels=True)[:2]
            states.append(FF.State(arity, max_leaves, n, FF.frontier_of(old, levels, n, arity, max_leaves), root))
        else:
            states.append(FF.State(arity, max_leaves))
        computed.append(FW.computed_levels(states[-1], add, digest) if add.shape[0] else None)
    out = [np.zeros_like(a) for a in seeded]
    for i, (t, p) in enumerate(zip(tid, lid)):
        if t >= len(before):
            w = FW.Witness(arity, D)
        else:
            seed = FW.Witness(arity, D, seeded[0][i], seeded[1][i], seeded[2][i], seeded[3][i])
            w = FW.refresh(seed, int(p), states[t], grow[t], digest, computed=computed[t])
        out[0][i], out[1][i], out[2][i], out[3][i] = w.leaf, w.siblings, w.positions, w.depth
    return out


# ---- 1. a witness for every leaf of a forest of every small transition ----
PAIRS = [(0, 0), (0, 1), (0, 5), (0, 20), (1, 0), (1, 1), (1, 3), (2, 2), (2, 20), (3, 1), (3, 13), (4, 0), (4, 1), (4, 12), (5, 11), (5, 20),
         (15, 1), (15, 2), (15, 20), (16, 0), (16, 1), (16, 4), (17, 15), (17, 20), (63, 1), (63, 2), (63, 20), (64, 0), (64, 1), (64, 17),
         (65, 0), (65, 20), (70, 19), (70, 20), (89, 1), (89, 2), (70, -3), (89, 0), (17, 6)]
REFUSED_TOO_LONG, REFUSED_DECREASING = PAIRS.index((89, 2)), PAIRS.index((70, -3))


@pytest.mark.parametrize("arity", [4, 2])
def test_a_witness_for_every_leaf_of_every_small_transition(gpu_ctx, oracle_mod, arity):
    """39 trees of 0 .. 89 leaves receive 0 .. 20 (two land exactly on max_leaves = 90, one is refused for n + m > 90, one for
    decreasing offsets): a witness for EVERY (t, p) with p < n' — the carried ones seeded by the openings call on the stored forest at
    n, the new ones holding garbage — and the bad ones: an unknown tree, p = n', leaves of both refused appends, a stale depth byte,
    an input 0xFF in a tree that grows and in one that does not"""
    import torch
    max_leaves, T = 90, len(PAIRS)
    D = TS.depth(max_leaves, arity)
    sizes = [p[0] for p in PAIRS]
    aoff = np.zeros(T + 1, dtype=np.int64)
    for t, (_, m) in enumerate(PAIRS):
        aoff[t + 1] = aoff[t] + m  # (the decrease of 3: the tree behind it takes leaves that an earlier tree took as well)
    n_add = int(aoff[-1]) + 3  # (so the appends accepted add up to no more than n_add: the sum rule refuses none of them)
    m, refused = FF.accepted_appends(sizes, aoff, n_add, max_leaves)
    assert [t for t in range(T) if refused[t]] == sorted((REFUSED_TOO_LONG, REFUSED_DECREASING))
    assert [a for (_, a), r in zip(PAIRS, refused) if not r] == [a for a, r in zip(m, refused) if not r]
    assert sum(n + a == max_leaves for n, a in zip(sizes, m)) >= 2
    flat, add = oracle_mod.fill_random(0xE00 + arity, sum(sizes)), oracle_mod.fill_random(0xE10 + arity, n_add)
    off = TS.offsets(sizes, dtype=np.int64)
    before = [flat[off[t]:off[t + 1]] for t in range(T)]
    grow = [add[aoff[t]:aoff[t] + m[t]] for t in range(T)]
    after = [np.concatenate(p) for p in zip(before, grow)]
    # the watch list
    tid = [t for t in range(T) for _ in range(sizes[t] + m[t])]
    lid = [p for t in range(T) for p in range(sizes[t] + m[t])]
    n_good = len(tid)
    special = {}  # index -> what is wrong with the input
    grown, idle = PAIRS.index((17, 20)), PAIRS.index((65, 0))
    for t, p, what in ((T, 0, "tree"), (T + 7, 3, "tree"), (0, 0, "p"), (grown, 37, "p"), (grown, 2 ** 40, "p"), (idle, 65, "p"),
                       (REFUSED_TOO_LONG, 89, "p"), (REFUSED_TOO_LONG, 90, "p"), (REFUSED_DECREASING, 70, "p"),
                       (grown, 5, "stale+1"), (grown, 16, "stale-1"), (PAIRS.index((15, 1)), 14, "stale+1"), (grown, 9, "0xFF"), (idle, 9, "0xFF"),
                       (grown, 5, "duplicate"), (grown, 30, "duplicate")):
        if what != "p" and what != "tree" and what != "duplicate":
            special[len(tid)] = what
        tid.append(t), lid.append(p)
    k = len(tid)
    assert k > 2 * 256 + 64
    order = np.random.default_rng(arity).permutation(k)  # any order
    tid, lid = np.asarray(tid)[order], np.asarray(lid, dtype=np.uint64)[order]
    special = {int(np.nonzero(order == i)[0][0]): what for i, what in special.items()}
    state, old = _state_of(gpu_ctx, arity, before, max_leaves)
    seeded = _stored_openings(gpu_ctx, arity, old, tid, lid)  # (bad where p >= n)
    rng = np.random.default_rng(100 + arity)
    for i in range(k):
        if tid[i] < T and sizes[tid[i]] <= lid[i]:  # not in the tree yet: garbage, a plausible depth byte included
            seeded[0][i], seeded[1][i] = rng.integers(0, 2 ** 63, 4), rng.integers(0, 2 ** 63, seeded[1][i].shape)
            seeded[2][i], seeded[3][i] = rng.integers(0, 256, D), rng.integers(0, D + 1)
    for i, what in special.items():
        seeded[3][i] = 0xFF if what == "0xFF" else int(seeded[3][i]) + (1 if what == "stale+1" else -1)
    w = Wits(arity, D, tid, lid)
    w.put(seeded)
    d_add, d_aoff = _torch(add), _torch(aoff.astype(np.uint64))
    plain = _copy_state(state)
    want_bad, want_hashed = _plain(gpu_ctx, plain, d_add, d_aoff)
    bad, hashed, bad_witness = _counters()
    w.append(gpu_ctx, state, d_add, d_aoff, bad, hashed, bad_witness)
    got = w.get()
    # the state and the counters: byte for byte the plain call's
    assert _same_state(state, plain) and int(bad) == int(want_bad) == 2 and int(hashed) == int(want_hashed)
    assert np.array_equal(_np(state.counts).astype(np.int64), np.asarray(sizes) + np.asarray(m))
    # the model, for every witness
    model = _model(oracle_mod, arity, D, max_leaves, before, grow, tid, lid, seeded)
    assert _differ(got, model).size == 0, [(int(tid[i]), int(lid[i])) for i in _differ(got, model)[:8]]
    # the openings call on a fresh stored build of the grown forest, for every witness whose input was as the call asks
    fresh = _stored_openings(gpu_ctx, arity, Old(gpu_ctx, arity, np.concatenate(after), TS.offsets([a.shape[0] for a in after]), max_leaves), tid, lid)
    plainly = np.array([i not in special for i in range(k)])
    differ = [i for i in _differ(got, fresh) if plainly[i]]
    assert differ == [], [(int(tid[i]), int(lid[i])) for i in differ[:8]]
    is_bad = got[3] == 0xFF
    assert int(is_bad.sum()) == k - n_good - 2 and int(bad_witness) == int(is_bad.sum())  # (the two duplicates are good ones)
    assert all(is_bad[i] for i, what in special.items()) and not is_bad[plainly & (fresh[3] != 0xFF)].any()
    for arr in got[:3]:  # a bad witness is all zero — but for the one of the idle tree, which stays as it came
        zero = [i for i in np.nonzero(is_bad)[0] if not (special.get(int(i)) == "0xFF" and tid[i] == idle)]
        assert not arr[zero].any()
    keep = [i for i, what in special.items() if what == "0xFF" and tid[i] == idle]
    assert len(keep) == 1 and all(np.array_equal(g[keep], s[keep]) for g, s in zip(got, seeded))
    # every good witness verifies against the state's roots, no bad one does
    assert np.array_equal(w.verify(gpu_ctx, state), (~is_bad).astype(np.uint8))
    assert w.canaries_intact()
    torch.cuda.synchronize()


# ---- 2. one set of witnesses carried through six appends ----
@pytest.mark.parametrize("arity", [4, 2])
def test_one_set_of_witnesses_carried_through_six_appends(gpu_ctx, oracle_mod, arity):
    """seven trees, appends of 1, 0, 3, 17, 1, 40 leaves with the trees taking turns (tree 6 never grows): the witnesses of every leaf
    the trees will ever hold are seeded once, out of the stored forest at the start, and only the call touches them afterwards"""
    max_leaves, steps = 90, (1, 0, 3, 17, 1, 40)
    D = TS.depth(max_leaves, arity)
    sizes = [0, 1, 5, 16, 17, 27, 9]
    T = len(sizes)
    adds = [[steps[(s + t) % 6] if t < 6 else 0 for t in range(T)] for s in range(6)]
    final = [n + sum(a[t] for a in adds) for t, n in enumerate(sizes)]
    assert max(final) <= max_leaves
    trees = [oracle_mod.fill_random(0xE20 + 16 * arity + t, final[t]) for t in range(T)]  # all leaves tree t will ever hold
    tid = np.array([t for t in range(T) for _ in range(final[t])])
    lid = np.array([p for t in range(T) for p in range(final[t])], dtype=np.uint64)
    state, old = _state_of(gpu_ctx, arity, [trees[t][:sizes[t]] for t in range(T)], max_leaves)
    w = Wits(arity, D, tid, lid)
    w.put(_stored_openings(gpu_ctx, arity, old, tid, lid))
    counts = list(sizes)
    for s in range(6):
        grow = [trees[t][counts[t]:counts[t] + adds[s][t]] for t in range(T)]
        before = w.get()
        bad, hashed, bad_witness = _counters()
        w.append(gpu_ctx, state, _torch(np.concatenate(grow)), _torch(TS.offsets(adds[s])), bad, hashed, bad_witness)
        counts = [n + a for n, a in zip(counts, adds[s])]
        got = w.get()
        now = [trees[t][:counts[t]] for t in range(T)]
        fresh = _stored_openings(gpu_ctx, arity, Old(gpu_ctx, arity, np.concatenate(now), TS.offsets(counts), max_leaves), tid, lid)
        assert _differ(got, fresh).size == 0, (s, [(int(tid[i]), int(lid[i])) for i in _differ(got, fresh)[:8]])
        idle = np.array([adds[s][t] == 0 for t in tid])
        assert idle.any() and _differ([g[idle] for g in got], [b[idle] for b in before]).size == 0, s
        in_tree = lid < np.asarray(counts, dtype=np.uint64)[tid]
        assert int(bad) == 0 and int(bad_witness) == int((~in_tree).sum()) and int(hashed) == sum(FF.n_hashed(n - a, a, arity) for n, a in zip(counts, adds[s]))
        assert np.array_equal(w.verify(gpu_ctx, state), in_tree.astype(np.uint8)), s
        assert w.canaries_intact(), s
    assert counts == final


# ---- 3. one larger tree ----
@pytest.mark.parametrize("arity", [4, 2])
def test_every_leaf_of_one_larger_tree_behind_a_small_one(gpu_ctx, oracle_mod, arity):
    """4^5 (arity 2: 2^10) leaves + 3,000 under max_leaves = 2^13, all 4,024 positions witnessed, behind a tree of 3 + 5 leaves: the runs
    of V_l span several blocks and start past the small tree's nodes in every level's values"""
    max_leaves, n, m = 2 ** 13, 1024, 3000
    D = TS.depth(max_leaves, arity)
    small, big = oracle_mod.fill_random(0xE40 + arity, 8), oracle_mod.fill_random(0xE50 + arity, n + m)
    tid = np.array([0] * 8 + [1] * (n + m))
    lid = np.array(list(range(8)) + list(range(n + m)), dtype=np.uint64)
    state, old = _state_of(gpu_ctx, arity, [small[:3], big[:n]], max_leaves)
    w = Wits(arity, D, tid, lid)
    w.put(_stored_openings(gpu_ctx, arity, old, tid, lid))
    bad, hashed, bad_witness = _counters()
    w.append(gpu_ctx, state, _torch(np.concatenate([small[3:], big[n:]])), _torch(np.array([0, 5, 5 + m], dtype=np.uint64)), bad, hashed, bad_witness)
    got = w.get()
    fresh = _stored_openings(gpu_ctx, arity, Old(gpu_ctx, arity, np.concatenate([small, big]), np.array([0, 8, 8 + n + m], dtype=np.uint64), max_leaves),
                             tid, lid)
    assert _differ(got, fresh).size == 0, [(int(tid[i]), int(lid[i])) for i in _differ(got, fresh)[:8]]
    assert int(bad) == 0 and int(bad_witness) == 0 and int(hashed) == FF.n_hashed(3, 5, arity) + FF.n_hashed(n, m, arity)
    assert bool((got[3] == TS.depth(n + m, arity))[8:].all()) and w.verify(gpu_ctx, state).all() and w.canaries_intact()


# ---- 4. the trivial sizes ----
@pytest.mark.parametrize("arity", [4, 2])
def test_no_witness_no_row_no_leaf_and_no_tree(gpu_ctx, oracle_mod, arity):
    import torch
    call = gpu_ctx.merkle4_forest_frontier_append_witness_device if arity == 4 else gpu_ctx.merkle2_forest_frontier_append_witness_device
    u8 = lambda *v: torch.tensor(v, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    leaves = oracle_mod.fill_random(0xE60 + arity, 40)
    # k == 0 is the plain call, with no witness buffer at all
    state, _ = _state_of(gpu_ctx, arity, [leaves[:5], leaves[5:5], leaves[5:22]], 90)
    plain = _copy_state(state)
    d_add, d_aoff = _torch(leaves[22:]), _torch(np.array([0, 7, 8, 18], dtype=np.uint64))
    want_bad, want_hashed = _plain(gpu_ctx, plain, d_add, d_aoff)
    bad, hashed, bad_witness = _counters()
    call(_tag(arity), state.counts, state.frontier, state.roots, 3, 90, d_add, d_aoff, None, None, 0, None, None, None, None, bad, hashed, bad_witness)
    assert _same_state(state, plain) and int(bad) == int(want_bad) and int(hashed) == int(want_hashed) and int(bad_witness) == 0
    # n_add == 0: nothing changes, the bad witnesses are marked and counted (one of them for the 0xFF it came with, in place)
    D = TS.depth(90, arity)
    tid, lid = [0, 0, 1, 2, 3, 0], [0, 12, 8, 27, 0, 3]  # (12, 27: p = n'; 8: past it; tree 3 is unknown)
    w = Wits(arity, D, tid, lid)
    seeded = [np.full(a.shape, 3, dtype=a.cpu().numpy().dtype) for a in (w.leaves, w.sib, w.pos, w.dep)]
    seeded[3][5] = 0xFF
    w.put(seeded)
    before = _copy_state(state)
    bad, hashed, bad_witness = _counters()
    w.append(gpu_ctx, state, None, _torch(np.zeros(4, dtype=np.uint64)), bad, hashed, bad_witness)
    got = w.get()
    assert _same_state(state, before) and int(bad) == 0 and int(hashed) == 0 and int(bad_witness) == 5
    assert all(np.array_equal(g[[0, 5]], s[[0, 5]]) for g, s in zip(got, seeded))  # in the tree: as they came
    assert not any(g[1:5].any() for g in got[:3]) and (got[3][1:5] == 0xFF).all() and w.canaries_intact()
    # D == 0 (max_leaves == 1): only leaves and depth bytes
    from poseidon252_amd import merkle
    one = merkle.ForestFrontier(gpu_ctx, 3, 1, arity)
    _plain(gpu_ctx, one, _torch(leaves[:1]), _torch(np.array([0, 0, 1, 1], dtype=np.uint64)))  # tree 1 holds a leaf
    tid, lid = _torch(np.array([0, 1, 2, 0, 3], np.uint32)), _torch(np.array([0, 0, 0, 1, 0], np.uint64))
    w_leaves = torch.full((5 + 2, 4), SENTINEL, dtype=torch.int64, device="cuda:0")
    w_dep = u8(9, 0, 9, 9, 9, CANARY, CANARY)
    w_leaves[1] = _torch(leaves[0])
    bad, hashed, bad_witness = _counters()
    call(_tag(arity), one.counts, one.frontier, one.roots, 3, 1, _torch(leaves[1:3]), _torch(np.array([0, 1, 1, 1], dtype=np.uint64)), tid, lid, 5,
         w_leaves[:5], None, None, w_dep[:5], bad, hashed, bad_witness)
    torch.cuda.synchronize()
    assert w_dep.tolist() == [0, 0, 0xFF, 0xFF, 0xFF, CANARY, CANARY] and int(bad_witness) == 3 and int(bad) == 0 and int(hashed) == 0
    want = np.zeros((5, 4), dtype=np.uint64)
    want[0], want[1] = leaves[1], leaves[0]
    assert np.array_equal(_np(w_leaves[:5]), want) and bool((w_leaves[5:] == SENTINEL).all()) and one.counts.tolist() == [1, 1, 0]
    ok = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.merkle_forest_ragged_verify_device(_tag(arity), w_leaves[:5], None, None, w_dep[:5], 0, tid, one.roots, 3, ok, 5, arity=arity)
    torch.cuda.synchronize()
    assert ok.tolist() == [1, 1, 0, 0, 0]
    # no tree at all: every witness is a bad one
    w = Wits(arity, D, [0, 1], [0, 5])
    bad, hashed, bad_witness = _counters()
    empty = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    call(_tag(arity), empty, empty, empty, 0, 90, None, empty, w.tid, w.lid, 2, w.leaves, w.sib, w.pos, w.dep, bad, hashed, bad_witness)
    got = w.get()
    assert int(bad_witness) == 2 and (got[3] == 0xFF).all() and not any(g.any() for g in got[:3]) and w.canaries_intact()


# ---- 5. the holders and the C++ mirror ----
def test_forest_witnesses_holder_follows_the_frontier(gpu_ctx, oracle_mod):
    import torch
    from poseidon252_amd import merkle
    sizes, adds = [3, 1, 17, 0], [2, 0, 5, 4]
    flat, add = oracle_mod.fill_random(0xE70, sum(sizes)), oracle_mod.fill_random(0xE71, sum(adds))
    off, aoff = TS.offsets(sizes, dtype=np.int64), TS.offsets(adds, dtype=np.int64)
    for arity in (4, 2):
        old = Old(gpu_ctx, arity, flat, TS.offsets(sizes), 17)
        state, _ = merkle.ForestFrontier.from_forest(gpu_ctx, old.d, old.d_off, 4, 17, old.d_lv, old.roots, max_leaves=70, arity=arity)
        # watched from the start (taken at the forest's own stride, kept at the state's wider one), and watched from their append on
        seen, n_bad = merkle.ForestWitnesses.from_openings(gpu_ctx, old.d, old.d_off, 4, 17, old.d_lv, [0, 2, 2, 1], [1, 0, 16, 0], max_leaves=70,
                                                           arity=arity)
        new = merkle.ForestWitnesses(gpu_ctx, 4, 70, arity, np.array([0, 2, 3, 3]), np.array([4, 21, 0, 4]))
        assert int(n_bad) == 0 and new.depths.tolist() == [0xFF] * 4 and seen.siblings.shape == (4, TS.depth(70, arity), arity - 1, 4)
        assert TS.depth(70, arity) > TS.depth(17, arity)
        for w, want_bad in ((seen, 0), (new, 1)):
            copy = _copy_state(state)
            out = copy.append(_torch(add), _torch(TS.offsets(adds)), witnesses=w)
            torch.cuda.synchronize()
            assert len(out) == 3 and int(out[0]) == 0 and int(out[2]) == want_bad
            assert w.verify(copy).tolist() == [1, 1, 1, 1 - want_bad]
        grown = [np.concatenate([flat[off[t]:off[t + 1]], add[aoff[t]:aoff[t + 1]]]) for t in range(4)]
        big = Old(gpu_ctx, arity, np.concatenate(grown), TS.offsets([g.shape[0] for g in grown]), 70)
        for w in (seen, new):
            fresh = _stored_openings(gpu_ctx, arity, big, _np(w.tree_ids), _np(w.leaf_ids))
            assert _differ([_np(w.leaves), _np(w.siblings), _np(w.positions), _np(w.depths)], fresh).size == 0
        assert len(state.append(_torch(add), _torch(TS.offsets(adds)))) == 2  # (without witnesses: as before)
        with pytest.raises(ValueError, match="the witnesses are of arity"):
            state.append(None, _torch(np.zeros(5, dtype=np.uint64)), witnesses=merkle.ForestWitnesses(gpu_ctx, 1, 31, arity, [0], [0]))
    with pytest.raises(ValueError, match="arity must be 4 or 2"):
        merkle.ForestWitnesses(gpu_ctx, 1, 70, 3, [0], [0])


def test_cpp_mirror_on_gpu(gpu_ctx, oracle_mod, tmp_path):
    run_cpp_mirror(build_cpp_mirror("test_forest_witness_api", tmp_path))
