"""One ragged Merkle forest carried through a long mixed sequence of forest calls: the host model, the plans and the runner that
tests/test_forest_walk_cpu.py (a numpy stand-in of the library, no GPU) and tests/test_forest_walk_gpu.py (the library) share.  A plain
helper module, imported as edgecases, pymodel and primcases are; no torch at module level.

The forest is built ONCE and never rebuilt: every update, append and resize reads what the call before it wrote (leaves, offsets,
levels, roots), and after every one of them openings and forest multiproofs are extracted and verified.  What is expected comes from
the oracle's single-tree builds over the host model's leaves (per tree, cached: a step re-hashes the trees it changed) and from the
numpy models of testsupport (forest_resize_model — with keep None the append's — for offsets and counters, dirty_nodes for an update's digests,
forest_multiproof_extract / forest_multiproof_counts for the shared proof) — never from the code under test.

  HostForest            arity, max_leaves and one (n_t, 4) uint64 array per tree: the bytes as handed in; update / resize in numpy
  plan(profile, arity)  the deterministic step list (made against the host forest alone) with the facts the conditions are checked on
  Walk / run            carries (d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots) from each call's outputs into the next
                        call's inputs on a backend with Context's methods, and compares after every step"""
import numpy as np

import edgecases as E
from testsupport.forestappend import KEEP_ALL, forest_resize_model
from testsupport.forestupdate import dirty_nodes
from helpers.forest import SENTINEL
from testsupport.multiproofmodel import forest_multiproof_counts, forest_multiproof_extract
from testsupport import treeshape as TS

SENT64 = np.uint64(SENTINEL & E.M64)
TAIL = 5            # rows of sentinel past what a call may use, in every output buffer
START = 3           # offsets[0] of the forest the build takes (a resize compacts: its offsets start at 0)
SCAN_TILE = 2048    # FOREST_APPEND_SCAN_TILE of csrc/forest_append.h
LANE_GROUPS = 8192  # the largest host-known bound the 8-lane digests take (coop8 of csrc/kernels.h)
ORACLE_CAP = 300    # changed trees of a `wide` step the oracle covers (plus the trees at the scan-tile borders)
RESIZES = ("rollback", "reorg", "drop", "keepnone")
KINDS = ("update", "append") + RESIZES

PROFILES = {
    # trees, random sizes lo .. hi, the designated trees' sizes, max_leaves before and after it grows, pairs of the two first updates
    "small": dict(trees=40, lo=0, hi=256, deep=300, s1=37, s0=20, sp=69, sp_keep=64, max_leaves=300, max_grown=1100, k1=60, k2=40, grow=8,
                  reads=24, seed=11, long=True),
    "wide": dict(trees=4110, lo=1, hi=20, deep=20, s1=13, s0=7, sp=19, sp_keep=16, max_leaves=20, max_grown=70, k1=9000, k2=3000, grow=3,
                 reads=150, seed=12, long=False),
}
# the designated trees (both profiles): cut to one leaf and grown again; cut to nothing, empty across an update, grown again; cut to a
# whole power of the arity; unchanged between two changed neighbours; the deepest; one leaf from the start; empty from the start
T_ONE, T_ZERO, T_POWER, T_LEFT, T_SAME, T_RIGHT, T_DEEP, T_LEAF, T_EMPTY = 3, 5, 7, 9, 10, 11, 12, 14, 16


def _empty():
    return np.zeros((0, 4), dtype=np.uint64)


def _unreduced(i):
    """a limb pattern at or above p (one of edgecases.PATTERNS)"""
    return E._PAT_RAW[E._BIG[i % len(E._BIG)]].copy()


def borders(n_trees):
    """the trees on each side of every scan-tile border inside a forest of n_trees"""
    return [t for b in range(SCAN_TILE, n_trees, SCAN_TILE) for t in (b - 1, b)]


# ---------------------------------------------------------------------------------------------- the host forest
class HostForest:
    """the reference state.  Expected roots and tree-major level blocks are the oracle's single-tree builds over the leaves mod p: an
    empty tree has a zero root and no storage, a one-leaf tree its leaf mod p as root and no storage; cached per tree"""

    def __init__(self, arity, max_leaves, trees):
        self.arity, self.max_leaves, self.tag = arity, int(max_leaves), E._mtag(arity)
        self.trees = [np.array(t, dtype=np.uint64).reshape(-1, 4) for t in trees]
        self._built = [None] * len(self.trees)

    @property
    def n_trees(self):
        return len(self.trees)

    def sizes(self):
        return [t.shape[0] for t in self.trees]

    def flat(self):
        return np.concatenate(self.trees + [_empty()])

    def update(self, tid, lid, new):
        """distinct (tid, lid) pairs get new[i]; a pair outside the forest (its tree empty, its leaf past the tree) writes nothing
        -> the mask of the good pairs"""
        tid, lid = np.asarray(tid, dtype=np.int64), np.asarray(lid, dtype=np.int64)
        assert len({(int(t), int(l)) for t, l in zip(tid, lid)}) == tid.size, "update pairs must be distinct"
        good = np.zeros(tid.size, dtype=bool)
        for i, (t, l) in enumerate(zip(tid, lid)):
            if 0 <= t < self.n_trees and 0 <= l < self.trees[t].shape[0]:
                self.trees[t][l] = new[i]
                self._built[t] = None
                good[i] = True
        return good

    def resize(self, keep, add, add_offsets, n_trees_new, max_leaves_new):
        """tree t keeps its first min(keep[t], n_t) leaves (keep None: all) and receives add[add_offsets[t]:add_offsets[t + 1]]; trees at
        or past n_trees_new are dropped, trees past the old forest start empty; keep None is the append -> the ids of the changed trees"""
        aoff = [int(x) for x in add_offsets]
        add = np.asarray(add, dtype=np.uint64).reshape(-1, 4)
        assert len(aoff) == n_trees_new + 1 and aoff[0] >= 0 and aoff[-1] <= add.shape[0] and all(b >= a for a, b in zip(aoff, aoff[1:]))
        trees, built, changed = [], [], []
        for t in range(n_trees_new):
            old = self.trees[t] if t < self.n_trees else _empty()
            k = old.shape[0] if keep is None else min(int(keep[t]) & KEEP_ALL, old.shape[0])
            m = aoff[t + 1] - aoff[t]
            assert k + m <= max_leaves_new, "the plans make no refused append"
            if k == old.shape[0] and m == 0:
                trees.append(old)
                built.append(self._built[t] if t < self.n_trees else None)
            else:
                trees.append(np.concatenate([old[:k], add[aoff[t]:aoff[t + 1]]]))
                built.append(None)
                changed.append(t)
        self.trees, self._built, self.max_leaves = trees, built, int(max_leaves_new)
        return changed

    def _oracle(self, t):
        leaves = self.trees[t]
        if leaves.shape[0] == 0:
            return np.zeros(4, dtype=np.uint64), _empty()
        if leaves.shape[0] == 1:
            return E.reduce_mod_p(leaves[:1])[0], _empty()
        root, levels, _ = E._otree(self.arity)(self.tag, E.reduce_mod_p(leaves), want_levels=True)
        return root, levels

    def ensure(self, ids=None):
        """the oracle's build of every listed tree (default: all) that changed since its last one"""
        stale = [t for t in (range(self.n_trees) if ids is None else ids) if self._built[t] is None]
        for t, b in zip(stale, E._pmap(self._oracle, stale) if len(stale) > 2 else [self._oracle(t) for t in stale]):
            self._built[t] = b

    def root(self, t):
        self.ensure([t])
        return self._built[t][0]

    def levels(self, t):
        self.ensure([t])
        return self._built[t][1]


# ---------------------------------------------------------------------------------------------- the plans
class Plan:
    def __init__(self, profile, arity, trees, max_leaves):
        self.profile, self.arity, self.trees, self.max_leaves, self.steps = profile, arity, trees, max_leaves, []

    def describe(self):
        """one line per step: kind, k / n_add, trees before and after, D"""
        out = ["plan %s arity %d: %d trees, %d leaves, max_leaves %d" % (self.profile, self.arity, len(self.trees), sum(t.shape[0] for t in self.trees),
                                                                         self.max_leaves)]
        for i, s in enumerate(self.steps, 1):
            what = "k=%d" % s["tid"].size if s["kind"] == "update" else "n_add=%d" % s["n_add"]
            out.append("  step %2d %-8s %-11s trees %d -> %d  leaves %d -> %d  D %d -> %d  view %s%s  reads %d" % (
                i, s["kind"], what, s["T_before"], s["T_after"], sum(s["sizes_before"]), sum(s["sizes_after"]), s["D_before"], s["D_after"],
                "whole(%d rows)" % s["n_view"] if s["whole"] else "sliced", "  sizing wrapper" if s["wrapper"] else "", s["r_tid"].size))
        return "\n".join(out)


class _Planner:
    def __init__(self, profile, arity, seed):
        self.cfg = cfg = PROFILES[profile]
        self.a, self.la = arity, 2 if arity == 4 else 1
        self.seed = cfg["seed"] if seed is None else seed
        self.rng = np.random.default_rng([self.seed, arity])
        self.draws = 0
        T = cfg["trees"]
        sizes = self.rng.integers(cfg["lo"], cfg["hi"] + 1, T)
        sizes[[T_ONE, T_ZERO, T_POWER, T_LEFT, T_SAME, T_RIGHT, T_DEEP, T_LEAF, T_EMPTY]] = [cfg["s1"], cfg["s0"], cfg["sp"], 12, 9, 12, cfg["deep"], 1, 0]
        for t in borders(T):
            sizes[t] = max(int(sizes[t]), 3)
        flat = self.draw(int(sizes.sum()))
        off = TS.offsets(sizes).astype(np.int64)
        trees = [flat[off[t]:off[t + 1]] for t in range(T)]
        self.H = HostForest(arity, cfg["max_leaves"], trees)
        self.P = Plan(profile, arity, [t.copy() for t in trees], cfg["max_leaves"])
        self.rows = START + int(sizes.sum()) + TAIL  # the carried leaf buffer, and where the forest's leaves end in it
        self.end = START + int(sizes.sum())
        self.wide = T > SCAN_TILE

    def draw(self, n):
        self.draws += 1
        return E.edge_draw(1000 * self.seed + 10 * self.draws + self.a, (n,))[0]

    def _common(self, kind, whole, wrapper):
        H = self.H
        return dict(kind=kind, whole=whole, wrapper=wrapper, T_before=H.n_trees, sizes_before=H.sizes(), maxl_before=H.max_leaves,
                    D_before=TS.depth(H.max_leaves, self.a), n_view=self.rows if whole else self.end, dead_rows=self.rows - self.end)

    def _done(self, s, changed, pairs):
        H, a = self.H, self.a
        s.update(T_after=H.n_trees, sizes_after=H.sizes(), maxl_after=H.max_leaves, D_after=TS.depth(H.max_leaves, a), changed=sorted(changed))
        # what the oracle covers: every tree in `small`; in `wide` the changed trees with the lowest ids and the trees at the tile borders
        if self.wide:
            cover = sorted(set(s["changed"][:ORACLE_CAP]) | {t for t in borders(H.n_trees)})
        else:
            cover = list(range(H.n_trees))
        s["cover"] = cover
        # the read phase: leaves the step just changed and random ones, in covered trees, strictly ascending in (tree, leaf)
        sizes, inside = s["sizes_after"], set(cover)
        full = [t for t in cover if sizes[t]]
        picks = {(int(t), int(l)) for t, l in pairs if t in inside and t < len(sizes) and l < sizes[t]}
        picks = set(sorted(picks)[:4 * self.cfg["reads"]])
        for t in borders(H.n_trees):
            picks |= {(t, 0), (t, sizes[t] - 1)}
        for t in self.rng.permutation(full)[:self.cfg["reads"]]:
            picks |= {(int(t), int(self.rng.integers(0, sizes[t]))), (int(t), sizes[t] - 1)}
        picks = sorted(picks)
        s["r_tid"], s["r_lid"] = np.array([p[0] for p in picks], dtype=np.uint32), np.array([p[1] for p in picks], dtype=np.uint64)
        s["bounds"].append(len(picks))
        self.P.steps.append(s)
        return s

    def update(self, k, whole=False, exclude=(), aimed_at_empty=(), siblings=0):
        """k leaves under k DISTINCT level-1 parents, every one-leaf tree, `siblings` second children, and pairs aimed at empty trees"""
        H, a, rng = self.H, self.a, self.rng
        s = self._common("update", whole, False)
        sizes = np.array(H.sizes(), dtype=np.int64)
        ok = np.ones(sizes.size, dtype=bool)
        ok[list(exclude)] = False
        parents = np.where((sizes > 1) & ok, (sizes + a - 1) // a, 0)
        tid = np.repeat(np.arange(sizes.size), parents)
        node = np.concatenate([np.arange(p) for p in parents if p] + [np.zeros(0, dtype=np.int64)])
        pick = np.sort(rng.permutation(tid.size)[:k])
        tid, node = tid[pick], node[pick]
        lid = np.minimum(node * a + rng.integers(0, a, size=tid.size), sizes[tid] - 1)
        s["k_parents"] = int(tid.size)
        sib = [i for i in range(tid.size) if (lid[i] ^ 1) < sizes[tid[i]]][:siblings]
        ones = np.nonzero((sizes == 1) & ok)[0]
        bad = np.array(list(aimed_at_empty), dtype=np.int64)
        assert all(sizes[t] == 0 for t in bad)
        tid = np.concatenate([tid, tid[sib], ones, bad])
        lid = np.concatenate([lid, lid[sib] ^ 1, np.zeros(ones.size + bad.size, dtype=np.int64)])
        new = self.draw(tid.size)
        at = tid.size - bad.size - ones.size
        for j in range(0, ones.size, 2):  # every other one-leaf tree gets limbs >= p
            new[at + j] = _unreduced(j + self.draws)
        s["unreduced_into_one_leaf"] = [int(ones[j]) for j in range(0, ones.size, 2)]
        order = rng.permutation(tid.size)  # (the call takes the pairs in any order)
        s["tid"], s["lid"], s["new"] = tid[order].astype(np.uint32), lid[order].astype(np.uint64), new[order]
        s["n_bad"], s["aimed_at_empty"] = int(bad.size), [int(t) for t in bad]
        fr = [(s["n_view"] >> (l * self.la)) + H.n_trees for l in range(1, s["D_before"] + 1)]
        s["bounds"] = [min(int(tid.size), b) for b in fr]
        good = H.update(s["tid"], s["lid"], s["new"])
        assert int((~good).sum()) == bad.size
        s["touched"] = sorted({int(t) for t in s["tid"][good]})
        return self._done(s, s["touched"], zip(s["tid"][good].tolist(), s["lid"][good].tolist()))

    def resize(self, kind, keep, m, max_new=None, wrapper=False, pure=False, one_leaf_new=()):
        """keep: {tree: kept count} over whole trees, or None (d_keep None); m: the appends, one per tree of the new forest"""
        H, a = self.H, self.a
        s = self._common(kind, False, wrapper)
        n_new = len(m)
        max_new = H.max_leaves if max_new is None else max_new
        aoff = TS.offsets(m)
        add = self.draw(int(aoff[-1]))
        for j, t in enumerate(one_leaf_new):  # a brand-new tree of exactly one leaf, its limbs >= p
            assert t >= H.n_trees and m[t] == 1
            add[int(aoff[t])] = _unreduced(j + self.draws)
        s["one_unreduced_leaf_new"] = list(one_leaf_new)
        if keep is None:
            s["keep"] = None
        else:
            s["keep"] = np.array([keep.get(t, KEEP_ALL) for t in range(n_new)], dtype=np.uint64)
        sizes = s["sizes_before"] + [0] * max(0, n_new - H.n_trees)
        s["k"] = [sizes[t] if keep is None else min(int(s["keep"][t]), sizes[t]) for t in range(n_new)]
        s["m"], s["n_add"], s["n_trees_new"], s["max_leaves_new"], s["pure"] = [int(x) for x in m], int(aoff[-1]), n_new, int(max_new), pure
        s["add"], s["add_offsets"] = (None, None) if pure else (add, aoff)
        assert not pure or s["n_add"] == 0
        N, T = s["n_view"] + s["n_add"], n_new
        s["dirty_bound_1"] = (s["n_add"] >> self.la) + 2 * T
        s["bounds"] = [min((s["n_add"] >> (l * self.la)) + 2 * T, (N >> (l * self.la)) + T) for l in range(1, TS.depth(min(max_new, max(N, 1)), a) + 1)]
        changed = H.resize(s["keep"], add, aoff, n_new, max_new)
        self.end = int(sum(H.sizes()))
        self.rows = N + (0 if wrapper else TAIL)
        pairs = [(t, l) for t in changed if H.trees[t].shape[0] for l in (0, H.trees[t].shape[0] - 1)]
        return self._done(s, changed, pairs)

    # ---- the ways a resize is drawn ----
    def cuts(self, share, least=1, spare=()):
        """{tree: kept count} for about `share` of the non-empty trees: at least `least` leaves stay"""
        sizes, rng = self.H.sizes(), self.rng
        first = (lambda n: max(least, n - 3)) if self.wide else (lambda n: least)  # (`wide` stays near its size: a few leaves come off)
        return {t: int(rng.integers(first(n), n + 1)) for t, n in enumerate(sizes) if n and t not in spare and rng.random() < share}

    def adds(self, n_new, share, most):
        """the appends of a new forest of n_new trees: 1 .. most leaves for about `share` of the old trees"""
        sizes, rng = self.H.sizes(), self.rng
        return [int(rng.integers(1, most + 1)) if t < len(sizes) and rng.random() < share else 0 for t in range(n_new)]


def plan(profile, arity, seed=None):
    """the deterministic step list of a profile ('small' | 'wide') and an arity (4 | 2), made against the host forest alone"""
    p = _Planner(profile, arity, seed)
    cfg, H, a, rng = p.cfg, p.H, arity, p.rng
    T = H.n_trees
    # 1: an update; 2: an append to the SAME trees, three brand-new trees (one unreduced leaf; five leaves; none), a deeper stride
    u = p.update(cfg["k1"], exclude=(T_SAME,), siblings=0 if p.wide else 10)
    m = [int(rng.integers(1, cfg["grow"] + 1)) if t in set(u["touched"]) else 0 for t in range(T)] + [1, 5, 0]
    p.resize("append", None, m, max_new=cfg["max_grown"], one_leaf_new=(T,))
    # 3: a pure rollback through the sizing wrapper: to one leaf, to nothing, to a whole power of the arity (nothing appended), every
    #    deepest tree to a shallower one, one tree unchanged between two changed ones
    sizes = H.sizes()
    deepest = max(TS.depth(n, a) for n in sizes)
    keep = p.cuts(0.5, spare=(T_SAME,))
    top = a ** (deepest - 1)  # (the largest tree one level shallower)
    keep.update({t: int(rng.integers(top - 3 if p.wide else 1, top + 1)) for t, n in enumerate(sizes) if TS.depth(n, a) == deepest})
    keep.update({T_ONE: 1, T_ZERO: 0, T_POWER: cfg["sp_keep"], T_LEFT: 5, T_RIGHT: sizes[T_RIGHT] - 1})
    keep.pop(T_SAME, None)
    p.resize("rollback", keep, [0] * H.n_trees, wrapper=True, pure=True)
    # 4: an update given the WHOLE buffer, dead rows behind the forest; one pair aimed at the tree that is empty now
    p.update(cfg["k2"], whole=True, aimed_at_empty=(T_ZERO,), siblings=0 if p.wide else 6)
    # 5: d_keep None: the empty tree and the one-leaf tree grow again, one new tree
    m = p.adds(H.n_trees + 1, 0.3, 4)
    m[T_ZERO], m[T_ONE], m[-1] = 4, 6, 3
    p.resize("keepnone", None, m)
    # 6: a reorg — cut and append in one call; 7: an update; 8: trailing trees dropped while others change
    m = p.adds(H.n_trees, 0.4, 4)
    p.resize("reorg", p.cuts(0.4), m)
    p.update(cfg["k2"] // 2, siblings=0 if p.wide else 6)
    n_new = H.n_trees - 7
    p.resize("drop", p.cuts(0.2), p.adds(n_new, 0.2, 3))
    if cfg["long"]:
        p.update(50, siblings=8)
        p.resize("append", None, p.adds(H.n_trees, 0.5, 9) + [2, 1], one_leaf_new=(H.n_trees + 1,))
        p.resize("rollback", p.cuts(0.6, least=0), [0] * H.n_trees)  # (not pure: d_add None, zero add offsets)
        p.update(40, whole=True, siblings=5, aimed_at_empty=[t for t, n in enumerate(H.sizes()) if n == 0][:2])
        p.resize("reorg", p.cuts(0.5, least=0), p.adds(H.n_trees + 1, 0.5, 6))
        p.resize("append", None, p.adds(H.n_trees, 0.3, 20))
        p.resize("drop", p.cuts(0.3), p.adds(H.n_trees - 4, 0.3, 5))
        p.resize("keepnone", None, p.adds(H.n_trees + 2, 0.4, 3))
        p.update(60, siblings=10)
    return p.P


# ---------------------------------------------------------------------------------------------- the runner
class GpuBackend:
    """Context's methods (the calls go to it unchanged), the two sizing wrappers of poseidon252_amd.merkle, and the only seam
    between numpy and the device: dev / host (edgecases._dev / _host)"""

    def __init__(self, ctx):
        self.ctx, self.dev, self.host = ctx, E._dev, E._host

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def forest_ragged_append(self, *args, **kw):
        from poseidon252_amd import merkle
        return merkle.forest_ragged_append(self.ctx, *args, **kw)

    def forest_ragged_resize(self, *args, **kw):
        from poseidon252_amd import merkle
        return merkle.forest_ragged_resize(self.ctx, *args, **kw)


class Walk:
    """one plan on one backend: build() once, then prepare(i) (uploads), launch(i) (library calls only: the step's call, then its read
    phase — nothing is read back in between) and check(i) (everything compared) for every step"""

    def __init__(self, plan, backend, check=True):
        self.plan, self.B, self.do_check, self.a = plan, backend, check, plan.arity
        self.tag = E._mtag(plan.arity)
        self.H = HostForest(plan.arity, plan.max_leaves, [t.copy() for t in plan.trees])
        self.wide = self.H.n_trees > SCAN_TILE
        self.run_same = E.Run(None).same
        self.fresh_only = []  # per step: the share of trees covered by the fresh build alone

    # ---- helpers ----
    def _full(self, *shape):
        return self.B.dev(np.full(shape, SENT64, dtype=np.uint64))

    def _zero(self, dtype):
        return self.B.dev(np.zeros(1, dtype=dtype))

    def _int(self, x):
        return int(np.asarray(self.B.host(x)).reshape(-1)[0])

    def _call(self, stem):
        return getattr(self.B, "merkle%d_forest_ragged_%s" % (self.a, stem))

    def _view(self, whole):
        return self.d_leaves if whole else self.d_leaves[:self.end]

    def _fail(self, i, kind, msg):
        raise AssertionError("step %d (%s): %s" % (i, kind, msg))

    # ---- step 0: the build ----
    def build(self):
        H, a, B = self.H, self.a, self.B
        sizes = H.sizes()
        self.off = TS.offsets(sizes, START)
        self.end = int(self.off[-1])
        buf = np.full((self.end + TAIL, 4), SENT64, dtype=np.uint64)
        buf[START:self.end] = H.flat()
        self.T, self.maxl, self.sentinel = H.n_trees, H.max_leaves, True
        self.d_leaves, self.d_off = B.dev(buf), B.dev(self.off)
        self.off_buf = self.d_off
        self.d_levels = self._full(TS.levels_bound(buf.shape[0], self.T, self.maxl, a) + TAIL, 4)
        self.roots_buf = self._full(self.T + TAIL, 4)
        self.d_roots = self.roots_buf[:self.T]
        bad = self._zero(np.int32)
        B.merkle_forest_ragged_device(self.tag, self.d_leaves, self.d_off, self.T, self.maxl, self.d_roots, self.d_levels, bad, arity=a)
        self.snap = None
        if self.do_check:
            try:
                assert self._int(bad) == sum(1 for n in sizes if n == 0), "n_bad of the build"
                cover = sorted(set(range(min(ORACLE_CAP, self.T))) | set(borders(self.T))) if self.wide else list(range(self.T))
                self._state(cover, True, None, None)
            except AssertionError as e:
                self._fail(0, "build", e)

    # ---- a step ----
    def prepare(self, i):
        """the step's inputs on the device, the host model moved on"""
        s, B, H, a = self.plan.steps[i - 1], self.B, self.H, self.a
        self.s = s
        c = self.c = dict(bad=self._zero(np.int32), hashed=self._zero(np.uint64))
        if self.do_check:
            H.ensure(sorted({int(t) for t in s["r_tid"] if t < H.n_trees}))
            c["old_roots"] = {int(t): H.root(int(t)).copy() for t in set(s["r_tid"].tolist()) if t < H.n_trees}
        c["sizes_before"], c["off_before"], c["n_view"] = H.sizes(), self.off, (self.rows() if s["whole"] else self.end)
        assert c["n_view"] == s["n_view"] and self.T == s["T_before"], "the carried buffers are not the ones the plan's bounds were worked out for"
        if s["kind"] == "update":
            c["tid"], c["lid"], c["new"] = B.dev(s["tid"]), B.dev(s["lid"]), B.dev(s["new"])
            c["good"] = H.update(s["tid"], s["lid"], s["new"])
        else:
            T2, n_add = s["n_trees_new"], s["n_add"]
            c["keep"] = None if s["keep"] is None else B.dev(s["keep"])
            c["add"] = B.dev(s["add"]) if n_add else None
            c["aoff"] = None if s["pure"] else B.dev(s["add_offsets"])
            if not s["wrapper"]:
                total = c["n_view"] + n_add
                c["out"] = (self._full(total + TAIL, 4), self._full(T2 + 1 + TAIL), self._full(TS.levels_bound(total, T2, s["max_leaves_new"], a) + TAIL, 4),
                            self._full(T2 + TAIL, 4))
            aoff = np.zeros(T2 + 1, dtype=np.uint64) if s["pure"] else s["add_offsets"]
            c["changed"] = H.resize(s["keep"], s["add"] if n_add else _empty(), aoff, T2, s["max_leaves_new"])
        # the read phase's inputs
        k = s["r_tid"].size
        sizes = H.sizes()
        c["r_tid"], c["r_lid"], c["k"] = B.dev(s["r_tid"]), B.dev(s["r_lid"]), k
        c["po_want"], c["mp_hashed_want"] = forest_multiproof_counts(sizes, s["r_tid"], s["r_lid"], a)
        c["old_pad"] = self._full(len(sizes), 4)  # the roots before the step, on the device; the sentinel for trees new in this step
        # the read phase's outputs (the forest's shape after the step is the model's: launch() allocates and uploads nothing of its own)
        T, maxl = len(sizes), H.max_leaves
        c["view_rows"] = c["n_view"] if s["kind"] == "update" else int(sum(sizes))
        c["bound"] = bound = getattr(B, "merkle%d_forest_ragged_multiproof_bound" % a)(c["view_rows"], T, maxl, k)
        assert int(c["po_want"][-1]) <= bound, "the model's proof is longer than the library's bound"
        c["o_bad"], c["mp_bad"] = B.dev(np.zeros(2, dtype=np.int32)), B.dev(np.zeros(2, dtype=np.int32))
        c["back"], c["ok"] = self._full(k, 4), B.dev(np.full((2, k), 7, dtype=np.uint8))
        c["mp_out"], c["mp_proof"], c["mp_po"] = self._full(k + TAIL, 4), self._full(bound + TAIL, 4), self._full(T + 1 + TAIL)
        c["mp_ok"], c["mp_roots"], c["mp_hashed"] = B.dev(np.full(T, 7, dtype=np.uint8)), self._full(T, 4), self._zero(np.uint64)

    def rows(self):
        return int(self.d_leaves.shape[0])

    def launch(self, i):
        """the step's call on the carried forest, then openings, re-hash, verify (against the carried roots and against the roots before
        the step), multiproof extract and verify — library calls and device copies only"""
        s, c, B, a = self.s, self.c, self.B, self.a
        m = min(len(c["sizes_before"]), len(self.H.sizes()))
        old_roots = self.d_roots
        if s["kind"] == "update":
            c["old_pad"][:m] = old_roots[:m]  # (the update rewrites d_roots in place)
            B.merkle_forest_ragged_update_device(self.tag, self._view(s["whole"]), self.d_off, self.T, self.maxl, self.d_levels, c["tid"], c["lid"],
                                                 c["new"], s["tid"].size, d_roots=self.d_roots, d_n_bad=c["bad"], d_n_hashed=c["hashed"], arity=a)
        else:
            T2, max_new = s["n_trees_new"], s["max_leaves_new"]
            old = (self.tag, self._view(False), self.d_off, self.T, self.maxl, self.d_levels)
            if s["wrapper"]:
                if s["kind"] == "append":
                    out = B.forest_ragged_append(*old, c["add"], c["aoff"], n_trees_new=T2, max_leaves_new=max_new, arity=a)
                else:
                    out = B.forest_ragged_resize(*old, d_keep=c["keep"], d_add=c["add"], d_add_offsets=c["aoff"], n_trees_new=T2, max_leaves_new=max_new,
                                                 arity=a)
                self.d_leaves, self.d_off, self.d_levels, self.roots_buf, c["bad"], c["hashed"] = out
                self.off_buf = self.d_off
            else:
                o = c["out"]
                keep = () if s["kind"] == "append" else (c["keep"],)
                self._call("append_device" if s["kind"] == "append" else "resize_device")(
                    *old, *keep, c["add"], c["aoff"], T2, max_new, o[0], o[1][:T2 + 1], o[2], o[3][:T2], c["bad"], c["hashed"])
                self.d_leaves, self.off_buf, self.d_levels, self.roots_buf = o
                self.d_off = self.off_buf[:T2 + 1]
            self.d_roots = self.roots_buf[:T2]
            self.sentinel = not s["wrapper"]
            self.T, self.maxl = T2, max_new
            self.off = TS.offsets(self.H.sizes())
            self.end = int(self.off[-1])
            c["old_pad"][:m] = old_roots[:m]
        # ---- the read phase, on the view the step's call had (an append / resize: the sliced view of its output) ----
        view, k, T, maxl = self._view(s["whole"]), c["k"], self.T, self.maxl
        assert int(view.shape[0]) == c["view_rows"]
        o_l, o_s, o_p, o_d, D = B.merkle_forest_ragged_openings_device(view, self.d_off, T, maxl, self.d_levels, c["r_tid"], c["r_lid"], k,
                                                                       d_n_bad=c["o_bad"][:1], arity=a)
        c["open"] = (o_l, o_s, o_p, o_d, D)
        B.merkle_path_ragged_device(self.tag, o_l, o_s, o_p, o_d, D, c["back"], k, d_n_bad=c["o_bad"][1:], arity=a)
        B.merkle_forest_ragged_verify_device(self.tag, o_l, o_s, o_p, o_d, D, c["r_tid"], self.d_roots, T, c["ok"][0], k, arity=a)
        B.merkle_forest_ragged_verify_device(self.tag, o_l, o_s, o_p, o_d, D, c["r_tid"], c["old_pad"], T, c["ok"][1], k, arity=a)
        bound, length = c["bound"], int(c["po_want"][-1])
        self._call("multiproof_device")(view, self.d_off, T, maxl, self.d_levels, c["r_tid"], c["r_lid"], k, c["mp_out"][:k],
                                        c["mp_proof"][:bound] if bound else None, c["mp_po"][:T + 1], c["mp_bad"][:1])
        # (the length is the model's: nothing is read back between the calls; the offsets are compared in check())
        self._call("multiproof_verify_device")(self.tag, self.d_off, c["view_rows"], T, maxl, c["r_tid"], c["r_lid"], c["mp_out"][:k], k,
                                               c["mp_proof"][:length] if length else None, length, c["mp_po"][:T + 1], self.d_roots, c["mp_ok"],
                                               c["mp_roots"], c["mp_hashed"], c["mp_bad"][1:])

    def check(self, i):
        if not self.do_check:
            return
        s = self.s
        try:
            self._check_step(s)
            self._check_reads(s)
        except AssertionError as e:
            self._fail(i, s["kind"], e)

    # ---- the comparisons ----
    def _state(self, cover, sentinel, untouched_from, changed):
        """the carried forest against the model and the oracle -> the host copies (leaves, offsets, levels, roots buffer)"""
        H, a, B = self.H, self.a, self.B
        sizes = H.sizes()
        leaves, off, levels, roots = (B.host(x) for x in (self.d_leaves, self.off_buf, self.d_levels, self.roots_buf))
        T = self.T
        assert T == H.n_trees and np.array_equal(off[:T + 1], self.off), "the offsets are not the model's"
        lo_, hi_ = int(self.off[0]), int(self.off[-1])
        if not np.array_equal(leaves[lo_:hi_], H.flat()):
            at = int(np.nonzero((leaves[lo_:hi_] != H.flat()).any(axis=1))[0][0])
            t = int(np.searchsorted(self.off.astype(np.int64) - lo_, at, side="right") - 1)
            raise AssertionError("the leaves are not the bytes handed in, first at tree %d leaf %d" % (t, at - int(self.off[t]) + lo_))
        lo = TS.block_starts(sizes, a)
        used = int(lo[-1])
        H.ensure(cover)
        want_roots = np.stack([H.root(t) for t in cover]) if cover else np.zeros((0, 4), dtype=np.uint64)
        want_lv = [H.levels(t) for t in cover]
        idx = np.concatenate([np.arange(lo[t], lo[t + 1]) for t in cover] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        got_lv = levels[idx]
        want = np.concatenate(want_lv + [_empty()])
        if not np.array_equal(got_lv, want):
            j = int(np.nonzero((got_lv != want).any(axis=1))[0][0])
            slot = int(idx[j])
            t = int(np.searchsorted(lo, slot, side="right") - 1)
            p, l = slot - int(lo[t]), 1
            for w in TS.level_widths(sizes[t], a):
                if p < w:
                    break
                p, l = p - w, l + 1
            raise AssertionError("the levels differ from the oracle, first at (tree %d, level %d, node %d)" % (t, l, p))
        self.run_same(got_lv, want, "levels")
        got_roots = roots[:T][cover]
        if not np.array_equal(got_roots, want_roots):
            t = cover[int(np.nonzero((got_roots != want_roots).any(axis=1))[0][0])]
            raise AssertionError("the roots differ from the oracle, first at (tree %d, level %d, node 0)" % (t, TS.depth(sizes[t], a)))
        self.run_same(got_roots, want_roots, "roots")
        # everything at or past the used lengths: still the sentinel behind an append / resize into sentinel buffers; as it was before
        # behind an in-place update
        if sentinel:
            assert (levels[used:] == SENT64).all(), "levels written at or past the used length %d" % used
            assert (leaves[hi_:] == SENT64).all(), "leaves written at or past offsets[-1]"
            assert (roots[T:] == SENT64).all() and (off[T + 1:] == SENT64).all(), "roots or offsets written past n_trees"
        if untouched_from is not None:
            p_leaves, _, p_levels, p_roots = untouched_from
            assert np.array_equal(levels[used:], p_levels[used:]), "the update wrote at or past the used length %d of d_levels" % used
            assert np.array_equal(leaves[hi_:], p_leaves[hi_:]) and np.array_equal(leaves[:lo_], p_leaves[:lo_]), "the update wrote outside the forest's leaves"
            assert np.array_equal(roots[T:], p_roots[T:]), "the update wrote past n_trees of d_roots"
        if self.snap is not None and changed is not None:  # the roots of trees the step did not touch: byte-identical to the previous step's
            same = np.array([t for t in range(min(T, self.snap[3].shape[0], self.snap_T)) if t not in changed], dtype=np.int64)
            diff = np.nonzero((roots[same] != self.snap[3][same]).any(axis=1))[0]
            assert diff.size == 0, "the root of tree %d, which the step did not touch, changed" % (int(same[diff[0]]) if diff.size else -1)
        if self.wide:  # the whole state byte for byte against a fresh build of the model's forest into sentinel buffers
            f_levels, f_roots = self._full(*levels.shape), self._full(*roots.shape)
            buf = np.full(leaves.shape, SENT64, dtype=np.uint64)
            buf[lo_:hi_] = H.flat()
            B.merkle_forest_ragged_device(self.tag, B.dev(buf), self.d_off, T, self.maxl, f_roots[:T], f_levels, None, arity=a)
            f_levels, f_roots = B.host(f_levels), B.host(f_roots)
            assert (f_levels[used:] == SENT64).all() and (f_roots[T:] == SENT64).all()
            assert np.array_equal(levels[:used], f_levels[:used]), "the levels differ from a fresh build of the same forest"
            assert np.array_equal(roots[:T], f_roots[:T]), "the roots differ from a fresh build of the same forest"
            if sentinel:
                assert np.array_equal(levels, f_levels) and np.array_equal(roots, f_roots)
        self.fresh_only.append(1.0 - len(cover) / max(T, 1))
        self.snap, self.snap_T = (leaves, off, levels, roots), T
        return self.snap

    def _check_step(self, s):
        c, a = self.c, self.a
        bad, hashed = self._int(c["bad"]), self._int(c["hashed"])
        if s["kind"] == "update":
            want_hashed = dirty_nodes(c["sizes_before"], s["tid"], s["lid"], a)
            want_bad, changed = int((~c["good"]).sum()), set(s["touched"])
            prev = self.snap
        else:
            M = forest_resize_model(c["off_before"], c["n_view"], s["maxl_before"], s["keep"], np.zeros(s["n_trees_new"] + 1, np.uint64) if s["pure"]
                                    else s["add_offsets"], s["n_add"], s["max_leaves_new"], a)
            assert M["n_new"] == self.H.sizes() and not any(M["refused"]), "the host forest and forest_resize_model disagree"
            want_hashed, want_bad, changed, prev = M["n_hashed"], M["n_bad"], set(c["changed"]), None
        self._state(s["cover"], self.sentinel and s["kind"] != "update", prev, changed)
        assert bad == want_bad, "n_bad %d, the model's %d" % (bad, want_bad)
        assert hashed == want_hashed, "n_hashed %d, the model's %d" % (hashed, want_hashed)

    def _check_reads(self, s):
        c, a, B, H = self.c, self.a, self.B, self.H
        sizes, T, k = H.sizes(), self.T, c["k"]
        tid, lid = s["r_tid"].astype(np.int64), s["r_lid"].astype(np.int64)
        H.ensure(sorted(set(tid.tolist())))
        want_roots = np.stack([H.root(int(t)) for t in tid])
        raw = np.stack([H.trees[int(t)][int(l)] for t, l in zip(tid, lid)])
        # openings: the leaves' bytes, the depths, the re-hash by the library and by the oracle, the two verdicts
        o_l, o_s, o_p, o_d, D = c["open"]
        assert D == TS.depth(self.maxl, a) and B.host(c["o_bad"]).tolist() == [0, 0], "openings: the stride, or a bad opening"
        assert np.array_equal(B.host(o_l), raw), "openings: the leaves are not the bytes handed in"
        depths = np.array([TS.depth(sizes[int(t)], a) for t in tid], dtype=np.int64)
        assert np.array_equal(B.host(o_d).astype(np.int64), depths), "openings: the depths are not depth(n_t)"
        self.run_same(B.host(c["back"]), want_roots, "openings re-hashed")
        sib, pos = B.host(o_s).reshape(k, D, a - 1, 4), B.host(o_p).reshape(k, D)
        assert np.array_equal(E.rehash(H.tag, a, E.reduce_mod_p(raw), E.reduce_mod_p(sib), pos, depths), want_roots), "openings: the oracle's re-hash"
        ok = B.host(c["ok"])
        assert (ok[0] == 1).all(), "opening %d does not verify against the carried d_roots" % int(np.argmin(ok[0] == 1))
        for j, t in enumerate(tid.tolist()):
            if t in c["old_roots"]:  # (the tree id existed before the step)
                same = np.array_equal(c["old_roots"][t], want_roots[j])
                assert int(ok[1][j]) == int(same), "opening %d of tree %d against the roots before the step: verdict %d, roots %s" % (
                    j, t, int(ok[1][j]), "equal" if same else "differ")
        # the shared proof: bytes, offsets, verdicts, recomputed roots, digests
        lo = TS.block_starts(sizes, a)
        model_lv = np.zeros((int(lo[-1]), 4), dtype=np.uint64)
        for t in set(tid.tolist()):
            model_lv[lo[t]:lo[t + 1]] = H.levels(t)
        want_out, want_proof, want_po = forest_multiproof_extract(H.flat(), TS.offsets(sizes).astype(np.int64), model_lv, tid, lid, a)
        assert np.array_equal(want_po, c["po_want"])
        length = int(want_po[-1])
        po, proof, out = B.host(c["mp_po"]), B.host(c["mp_proof"]), B.host(c["mp_out"])
        assert B.host(c["mp_bad"]).tolist() == [0, 0], "multiproof: a bad pair"
        assert np.array_equal(po[:T + 1], want_po) and (po[T + 1:] == SENT64).all(), "multiproof: proof_offsets"
        assert np.array_equal(out[:k], want_out) and (out[k:] == SENT64).all(), "multiproof: the leaves"
        assert np.array_equal(proof[:length], want_proof) and (proof[length:] == SENT64).all(), "multiproof: the proof's bytes"
        has = np.zeros(T, dtype=bool)
        has[tid] = True
        assert np.array_equal(B.host(c["mp_ok"]).astype(np.int64), has.astype(np.int64)), "multiproof-verify: 1 exactly for the trees that have a pair"
        ids = np.nonzero(has)[0]
        self.run_same(B.host(c["mp_roots"])[ids], np.stack([H.root(int(t)) for t in ids]), "multiproof d_roots_out")
        assert self._int(c["mp_hashed"]) == c["mp_hashed_want"], "multiproof-verify: n_hashed"

    def final(self):
        """the last state against the oracle on EVERY tree"""
        if self.do_check:
            try:
                self._state(list(range(self.T)), False, None, None)
            except AssertionError as e:
                self._fail(len(self.plan.steps), "final", e)


def run(plan, backend, check=True, before_step=None):
    """the whole plan on the backend -> the Walk (its fresh_only: per checked state, the share of trees the fresh build alone covers)"""
    w = Walk(plan, backend, check)
    w.build()
    for i in range(1, len(plan.steps) + 1):
        if before_step:
            before_step(i)
        w.prepare(i)
        w.launch(i)
        w.check(i)
    w.final()
    return w
