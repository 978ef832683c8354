"""The forest walk (tests/forestwalk.py) without a GPU: the conditions its plans must meet, asserted on the plans themselves; the host
forest's resize against the numpy models of testsupport/ at every step; the runner on HostBackend, a numpy-and-oracle stand-in with the
call surface of Context; and four stand-ins that are each wrong in one way, which the runner must reject AT the step in which the
fault first acts."""
import sys

import numpy as np
import pytest

import edgecases as E
import forestwalk as W
from testsupport.forestappend import forest_append_model, forest_resize_model, good_leaf_counts, model_leaves
from forestwalk import RESIZES
from testsupport.multiproofmodel import forest_multiproof_bound, forest_multiproof_counts, forest_multiproof_extract, forest_multiproof_roots
from testsupport import treeshape as TS

_PLANS = {}


def _plan(profile, arity):
    if (profile, arity) not in _PLANS:
        _PLANS[(profile, arity)] = W.plan(profile, arity)
    return _PLANS[(profile, arity)]


# ---------------------------------------------------------------------------------------------- 1. the plans
@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("profile", ["small", "wide"])
def test_plans_meet_their_conditions(profile, arity):
    P = _plan(profile, arity)
    print(P.describe())
    S, a = P.steps, arity
    assert W.plan(profile, arity).describe() == P.describe()  # deterministic
    held = {}

    def holds(number, what, ok):
        held[number] = bool(ok)
        print("  condition %2d %-5s %s" % (number, "holds" if ok else "FAILS", what))
    pairs = list(zip(S, S[1:]))
    is_resize = lambda s: s["kind"] in RESIZES  # noqa: E731
    size = lambda s, t, when: (s["sizes_" + when][t] if t < len(s["sizes_" + when]) else 0)  # noqa: E731
    kinds = {s["kind"] for s in S}
    holds(1, "every step kind occurs, a pure rollback (d_add and d_add_offsets None) among them",
          kinds == set(W.KINDS) and any(s["kind"] == "rollback" and s["pure"] and s["add"] is None and s["add_offsets"] is None for s in S)
          and any(s["kind"] == "drop" and s["T_after"] < s["T_before"] for s in S) and any(s["kind"] == "keepnone" and s["keep"] is None for s in S)
          and any(s["kind"] == "reorg" and any(k < n and m for k, n, m in zip(s["k"], s["sizes_before"], s["m"])) for s in S)
          and any(s["kind"] == "append" and s["T_after"] > s["T_before"] for s in S))
    holds(2, "openings and the multiproof follow every mutating kind", all(s["r_tid"].size > 0 for s in S) and {s["kind"] for s in S if s["r_tid"].size} == kinds)
    holds(3, "an update directly follows a resize with dead rows and is given the whole buffer",
          any(is_resize(p) and s["kind"] == "update" and s["whole"] and s["dead_rows"] > 0 and s["n_view"] > sum(s["sizes_before"]) for p, s in pairs))
    holds(4, "elsewhere a call is given the sliced view", any(not s["whole"] for s in S if s["kind"] == "update") and any(not s["whole"] for s in S if is_resize(s)))
    holds(5, "an append directly follows an update of the same trees",
          any(p["kind"] == "update" and s["kind"] == "append" and {t for t in range(s["T_before"]) if s["m"][t]} == set(p["touched"]) for p, s in pairs))
    holds(6, "a resize directly follows an append", any(p["kind"] == "append" and is_resize(s) for p, s in pairs))
    T_all = max(s["T_after"] for s in S)

    def history(t):
        return [size(S[0], t, "before")] + [size(s, t, "after") for s in S]
    holds(7, "a tree goes from more than one leaf to exactly one, and grows again",
          any(any(h[i] > 1 and h[i + 1] == 1 and max(h[i + 2:] + [0]) > 1 for i in range(len(h) - 1)) for h in map(history, range(T_all))))
    ok8 = False
    for i, s in enumerate(S):
        for t in (range(s["T_before"]) if is_resize(s) else ()):
            if size(s, t, "before") > 0 and size(s, t, "after") == 0:
                j = i + 1
                aimed = False
                while j < len(S) and size(S[j], t, "after") == 0 and t < S[j]["T_after"]:
                    aimed |= S[j]["kind"] == "update" and t in S[j]["aimed_at_empty"] and S[j]["n_bad"] >= 1
                    j += 1
                ok8 |= aimed and j < len(S) and S[j]["kind"] != "update" and S[j]["m"][t] > 0
    holds(8, "a tree is cut to nothing, is aimed at by an update while empty (counted in n_bad), and is appended to again", ok8)
    powers = {a ** h for h in range(1, 12)}
    holds(9, "a tree is cut with m = 0 to exactly arity^h leaves, h >= 1",
          any(is_resize(s) and any(m == 0 and k < n and k in powers for k, n, m in zip(s["k"], s["sizes_before"], s["m"])) for s in S))
    holds(10, "a tree is unchanged by a resize that changes its neighbours on both sides",
          any(is_resize(s) and any(t not in s["changed"] and size(s, t, "after") and t - 1 in s["changed"] and t + 1 in s["changed"]
                                   for t in range(1, s["T_after"] - 1)) for s in S))
    holds(11, "max_leaves grows so that the stride D grows", any(s["maxl_after"] > s["maxl_before"] and s["D_after"] > s["D_before"] for s in S))
    deepest = lambda sizes: max(TS.depth(n, a) for n in sizes)  # noqa: E731
    holds(12, "the deepest actual tree gets shallower while D stays",
          any(deepest(s["sizes_after"]) < deepest(s["sizes_before"]) and s["D_after"] == s["D_before"] for s in S))
    ok13 = False
    for s in S:
        if s["kind"] == "update":
            for t, v in zip(s["tid"], s["new"]):
                ok13 |= s["sizes_before"][t] == 1 and not bool(E.is_reduced(v))
    holds(13, "an update writes limbs >= p into a one-leaf tree", ok13)
    ok14 = False
    for s in S:
        if s["kind"] == "append":
            for t in range(s["T_before"], s["T_after"]):
                ok14 |= s["m"][t] == 1 and not bool(E.is_reduced(s["add"][int(s["add_offsets"][t])]))
    holds(14, "an append gives a brand-new tree exactly one leaf with limbs >= p", ok14)
    if profile == "small":
        holds(15, "every host-known per-level bound stays <= 8,192", max(b for s in S for b in s["bounds"]) <= W.LANE_GROUPS)
        assert len(S) >= 16 and 30 <= len(P.trees) <= 50 and max(t.shape[0] for t in P.trees) <= 320 and min(t.shape[0] for t in P.trees) == 0
    else:
        ups = [s for s in S if s["kind"] == "update"]
        holds(16, "one update has k > 8,192 pairs under distinct level-1 parents, another k <= 8,192",
              any(s["k_parents"] > W.LANE_GROUPS and s["bounds"][0] > W.LANE_GROUPS for s in ups) and any(s["tid"].size <= W.LANE_GROUPS for s in ups))
        holds(17, "an append or resize with a level-1 dirty bound > 8,192 is followed by an update with k <= 8,192",
              any(p["kind"] != "update" and p["dirty_bound_1"] > W.LANE_GROUPS and p["bounds"][0] > W.LANE_GROUPS and s["kind"] == "update"
                  and s["tid"].size <= W.LANE_GROUPS for p, s in pairs))
        holds(18, "multiproof pairs fall on both sides of every 2,048-tree tile border",
              all(W.borders(s["T_after"]) and set(W.borders(s["T_after"])) <= set(s["r_tid"].tolist()) for s in S))
        sizes0 = [t.shape[0] for t in P.trees]
        level1 = sum(TS.level_widths(n, a)[0] for n in sizes0 if n > 1)
        assert len(S) >= 6 and len(sizes0) > 2 * W.SCAN_TILE and level1 > W.LANE_GROUPS and 35000 <= sum(sizes0) <= 50000
        assert all(s["T_after"] > 2 * W.SCAN_TILE + 1 for s in S) and all(35000 <= sum(s["sizes_after"]) <= 60000 for s in S)
        assert any(s["kind"] == "append" and s["dirty_bound_1"] > W.LANE_GROUPS for s in S)
    assert sum(1 for s in S if s["wrapper"]) == 1
    for s in S:  # the reads: strictly ascending pairs inside non-empty trees, the changed leaves among them
        key = s["r_tid"].astype(np.int64) * (1 << 40) + s["r_lid"].astype(np.int64)
        assert (np.diff(key) > 0).all() and all(l < s["sizes_after"][t] for t, l in zip(s["r_tid"], s["r_lid"]))
        assert set(s["r_tid"].tolist()) & set(s["changed"])
    assert all(held.values()), "conditions that fail: %s" % sorted(n for n, ok in held.items() if not ok)


# ---------------------------------------------------------------------------------------------- 2. the host forest against the models
@pytest.mark.parametrize("arity", [4, 2])
def test_host_forest_agrees_with_the_numpy_models(arity):
    P = _plan("small", arity)
    H = W.HostForest(arity, P.max_leaves, [t.copy() for t in P.trees])
    n_checked = 0
    for i, s in enumerate(P.steps, 1):
        if s["kind"] == "update":
            H.update(s["tid"], s["lid"], s["new"])
            continue
        sizes, flat, maxl = H.sizes(), H.flat(), H.max_leaves
        off = TS.offsets(sizes)
        aoff = np.zeros(s["n_trees_new"] + 1, np.uint64) if s["pure"] else s["add_offsets"]
        add = s["add"] if s["n_add"] else np.zeros((0, 4), np.uint64)
        H.resize(s["keep"], add, aoff, s["n_trees_new"], s["max_leaves_new"])
        M = forest_resize_model(off, flat.shape[0], maxl, s["keep"], aoff, s["n_add"], s["max_leaves_new"], arity)
        assert M["n_new"] == H.sizes() == s["sizes_after"] and M["offsets_new"].tolist() == TS.offsets(H.sizes()).tolist(), i
        assert np.array_equal(model_leaves(M, flat, add), H.flat()), i
        assert M["n_bad"] == sum(1 for n in H.sizes() if n == 0) and M["k"] == s["k"] and M["m"] == s["m"], i
        direct = 0
        for n, k, m in zip(sizes + [0] * s["n_trees_new"], M["k"], M["m"]):
            if k != n or m:
                direct += sum(-(-(k + m) // arity ** l) - k // arity ** l for l in range(1, TS.depth(k + m, arity) + 1))
        assert M["n_hashed"] == direct, (i, M["n_hashed"], direct)
        if s["keep"] is None and s["n_trees_new"] >= len(sizes):
            A = forest_append_model(off, flat.shape[0], maxl, aoff, s["n_add"], s["max_leaves_new"], arity)
            assert A["n_new"] == M["n_new"] and A["n_hashed"] == M["n_hashed"] and A["n_bad"] == M["n_bad"], i
            assert np.array_equal(A["leaf_src"], M["leaf_src"]) and np.array_equal(A["node_src"], M["node_src"]), i
        n_checked += 1
    assert n_checked >= 9


# ---------------------------------------------------------------------------------------------- 3. the stand-in
def _tree(tag, arity, raw):
    if raw.shape[0] == 0:
        return np.zeros(4, np.uint64), np.zeros((0, 4), np.uint64)
    if raw.shape[0] == 1:
        return E.reduce_mod_p(raw[:1])[0], np.zeros((0, 4), np.uint64)
    root, levels, _ = E._otree(arity)(tag, E.reduce_mod_p(raw), want_levels=True)
    return root, levels


def _level_start(n, l, arity):
    return sum(TS.level_widths(n, arity)[:l - 1])


class HostBackend:
    """the call surface the runner uses, in numpy and the oracle: an in-place update that writes its dirty nodes only, an out-of-place
    append / resize that moves the clean nodes and writes nothing past what it uses, openings, re-hash, verify, the shared proof.
    fault = (name, n): wrong in one way from the n-th call of that kind on —
      'stale_top'   update leaves the top node of one touched tree stale
      'copied'      resize copies instead of re-hashing the one dirty node of level 1 of a cut tree
      'raw_root'    append writes a new one-leaf tree's root as its raw bytes instead of mod p
      'past_used'   update writes one scalar past the used length of d_levels"""

    def __init__(self, fault=None):
        self.fault, self.calls = fault, {"update": 0, "resize": 0, "append": 0}
        self.dev = lambda a: np.array(a, copy=True)
        self.host = lambda a: np.array(a, copy=True)

    def _acts(self, name, kind):
        return self.fault is not None and self.fault[0] == name and self.calls[kind] >= self.fault[1]

    # ---- build ----
    def merkle_forest_ragged_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_roots, d_levels=None, d_n_bad=None, arity=4):
        sizes = good_leaf_counts(d_offsets, d_leaves.shape[0], max_leaves)
        lo = TS.block_starts(sizes, arity)
        built = E._pmap(lambda t: _tree(tag, arity, d_leaves[int(d_offsets[t]):int(d_offsets[t]) + sizes[t]]), range(n_trees))
        for t, (root, lv) in enumerate(built):
            d_roots[t] = root
            if d_levels is not None:
                d_levels[lo[t]:lo[t + 1]] = lv
        if d_n_bad is not None:
            d_n_bad[0] += sum(1 for n in sizes if n == 0)

    # ---- update ----
    def merkle_forest_ragged_update_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, d_new_leaves, k,
                                           d_roots=None, d_n_bad=None, d_n_hashed=None, arity=4):
        self.calls["update"] += 1
        sizes = good_leaf_counts(d_offsets, d_leaves.shape[0], max_leaves)
        lo = TS.block_starts(sizes, arity)
        dirty, bad = set(), 0
        for i in range(k):
            t, l = int(d_tree_ids[i]), int(d_leaf_ids[i])
            if t >= n_trees or l >= sizes[t]:
                bad += 1
                continue
            d_leaves[int(d_offsets[t]) + l] = d_new_leaves[i]
            for lv in range(1, TS.depth(sizes[t], arity) + 1):
                dirty.add((t, lv, l // arity ** lv))
        touched = sorted({int(t) for t in d_tree_ids[:k] if t < n_trees and sizes[t]})
        built = dict(zip(touched, E._pmap(lambda t: _tree(tag, arity, d_leaves[int(d_offsets[t]):int(d_offsets[t]) + sizes[t]]), touched)))
        stale = None
        if self._acts("stale_top", "update"):
            stale = next(t for t in touched if sizes[t] > arity)
        for t, lv, j in dirty:
            if t == stale and lv == TS.depth(sizes[t], arity):
                continue
            d_levels[lo[t] + _level_start(sizes[t], lv, arity) + j] = built[t][1][_level_start(sizes[t], lv, arity) + j]
        for t in touched:
            if d_roots is not None and t != stale:
                d_roots[t] = built[t][0]
        if self._acts("past_used", "update"):
            d_levels[lo[-1]] = np.array([1, 0, 0, 0], np.uint64)
        if d_n_bad is not None:
            d_n_bad[0] += bad
        if d_n_hashed is not None:
            d_n_hashed[0] += len(dirty)

    # ---- append / resize ----
    def _resize(self, kind, tag, arity, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets, n_trees_new, max_new, d_leaves_new,
                d_offsets_new, d_levels_new, d_roots, d_n_bad, d_n_hashed):
        self.calls[kind] += 1
        old = good_leaf_counts(d_offsets, d_leaves.shape[0], max_leaves) if n_trees else []
        lo_old = TS.block_starts(old, arity)
        n_add = d_add.shape[0] if d_add is not None else 0
        assert d_leaves_new.shape[0] >= d_leaves.shape[0] + n_add and d_offsets_new.shape[0] == n_trees_new + 1 and d_roots.shape[0] == n_trees_new
        new, ks, ms = [], [], []
        for t in range(n_trees_new):
            n = old[t] if t < n_trees else 0
            k = n if d_keep is None else min(int(d_keep[t]), n)
            lo, hi = int(d_add_offsets[t]), int(d_add_offsets[t + 1])
            assert lo <= hi <= n_add and k + hi - lo <= max_new  # (the plans make no refused append)
            at = int(d_offsets[t]) if t < n_trees else 0
            new.append(np.concatenate([d_leaves[at:at + k], d_add[lo:hi] if hi > lo else np.zeros((0, 4), np.uint64)]))
            ks.append(k)
            ms.append(hi - lo)
        sizes = [x.shape[0] for x in new]
        off, lo_new = TS.offsets(sizes), TS.block_starts(sizes, arity)
        assert d_levels_new.shape[0] >= lo_new[-1]
        changed = [t for t in range(n_trees_new) if ms[t] or ks[t] != (old[t] if t < n_trees else 0)]
        built = dict(zip(changed, E._pmap(lambda t: _tree(tag, arity, new[t]), changed)))
        copied = None
        if self._acts("copied", "resize"):
            copied = next(t for t in changed if ms[t] == 0 and ks[t] % arity and ks[t] > arity)
        hashed = 0
        for t in range(n_trees_new):
            d_leaves_new[int(off[t]):int(off[t + 1])] = new[t]
            n, k = sizes[t], ks[t]
            if t not in built and t < n_trees:  # unchanged: moved whole
                d_levels_new[lo_new[t]:lo_new[t + 1]] = d_levels[lo_old[t]:lo_old[t + 1]]
            elif t in built:
                at, n_old = int(lo_new[t]), old[t] if t < n_trees else 0
                for l, w in enumerate(TS.level_widths(n, arity), 1):
                    clean = k // arity ** l
                    src = int(lo_old[t]) + _level_start(n_old, l, arity) if clean else 0
                    d_levels_new[at:at + clean] = d_levels[src:src + clean]
                    d_levels_new[at + clean:at + w] = built[t][1][at - int(lo_new[t]) + clean:at - int(lo_new[t]) + w]
                    if t == copied and l == 1:
                        d_levels_new[at + clean] = d_levels[src + clean]
                    hashed += w - clean
                    at += w
            if n == 0:
                d_roots[t] = 0
            elif n == 1:
                d_roots[t] = new[t][0] if (self._acts("raw_root", "append") and t >= n_trees) else E.reduce_mod_p(new[t][:1])[0]
            else:
                d_roots[t] = d_levels_new[lo_new[t + 1] - 1]
        d_offsets_new[:] = off
        if d_n_bad is not None:
            d_n_bad[0] += sum(1 for n in sizes if n == 0)
        if d_n_hashed is not None:
            d_n_hashed[0] += hashed

    def _append_device(self, arity, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_add, d_add_offsets, n_trees_new, max_new, *out):
        self._resize("append", tag, arity, d_leaves, d_offsets, n_trees, max_leaves, d_levels, None, d_add, d_add_offsets, n_trees_new, max_new, *out)

    def _resize_device(self, arity, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets, n_trees_new, max_new, *out):
        self._resize("resize", tag, arity, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets, n_trees_new, max_new, *out)

    def merkle4_forest_ragged_append_device(self, *args):
        self._append_device(4, *args)

    def merkle2_forest_ragged_append_device(self, *args):
        self._append_device(2, *args)

    def merkle4_forest_ragged_resize_device(self, *args):
        self._resize_device(4, *args)

    def merkle2_forest_ragged_resize_device(self, *args):
        self._resize_device(2, *args)

    def _sized(self, call, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, keep, d_add, d_add_offsets, n_trees_new, max_leaves_new, arity):
        """the sizing wrappers of poseidon252_amd.merkle: exact-sized outputs, nothing behind them"""
        n_add = d_add.shape[0] if d_add is not None else 0
        if d_add_offsets is None:
            d_add_offsets = np.zeros(n_trees_new + 1, np.uint64)
        total = d_leaves.shape[0] + n_add
        out = (np.zeros((total, 4), np.uint64), np.zeros(n_trees_new + 1, np.uint64),
               np.zeros((TS.levels_bound(total, n_trees_new, max_leaves_new, arity), 4), np.uint64), np.zeros((n_trees_new, 4), np.uint64),
               np.zeros(1, np.int32), np.zeros(1, np.uint64))
        call(arity, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, *keep, d_add, d_add_offsets, n_trees_new, max_leaves_new, *out)
        return out

    def forest_ragged_append(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_add, d_add_offsets, n_trees_new=None, max_leaves_new=None,
                             arity=4):
        return self._sized(self._append_device, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, (), d_add, d_add_offsets, n_trees_new,
                           max_leaves_new, arity)

    def forest_ragged_resize(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep=None, d_add=None, d_add_offsets=None, n_trees_new=None,
                             max_leaves_new=None, arity=4):
        return self._sized(self._resize_device, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, (d_keep,), d_add, d_add_offsets, n_trees_new,
                           max_leaves_new, arity)

    # ---- openings ----
    def merkle_forest_ragged_openings_device(self, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k, out=None, d_n_bad=None,
                                             arity=4):
        sizes = good_leaf_counts(d_offsets, d_leaves.shape[0], max_leaves)
        lo, D = TS.block_starts(sizes, arity), TS.depth(max_leaves, arity)
        lv, sib = np.zeros((k, 4), np.uint64), np.zeros((k, D, arity - 1, 4), np.uint64)
        pos, dep = np.zeros((k, D), np.uint8), np.zeros(k, np.uint8)
        for i in range(k):
            t, idx = int(d_tree_ids[i]), int(d_leaf_ids[i])
            assert t < n_trees and idx < sizes[t]  # (the plans ask for no bad opening)
            nodes = d_leaves[int(d_offsets[t]):int(d_offsets[t]) + sizes[t]]
            lv[i], dep[i], at = nodes[idx], TS.depth(sizes[t], arity), int(lo[t])
            for l, w in enumerate(TS.level_widths(sizes[t], arity)):
                pos[i, l] = idx % arity
                others = [c for c in range(idx - idx % arity, idx - idx % arity + arity) if c != idx]
                for j, c in enumerate(others):
                    if c < nodes.shape[0]:
                        sib[i, l, j] = nodes[c]
                nodes, at, idx = d_levels[at:at + w], at + w, idx // arity
        return lv, sib, pos, dep, D

    def _rehash(self, tag, arity, lv, sib, pos, dep, D, k):
        return E.rehash(tag, arity, E.reduce_mod_p(lv), E.reduce_mod_p(np.asarray(sib).reshape(k, D, arity - 1, 4)), np.asarray(pos).reshape(k, D),
                        np.asarray(dep).astype(np.int64))

    def merkle_path_ragged_device(self, tag, d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_roots, k, d_n_bad=None, arity=4):
        d_roots[:k] = self._rehash(tag, arity, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k)

    def merkle_forest_ragged_verify_device(self, tag, d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_tree_ids, d_roots, n_trees, d_ok, k,
                                           arity=4):
        got = self._rehash(tag, arity, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k)
        d_ok[:k] = (got == d_roots[np.asarray(d_tree_ids[:k], np.int64)]).all(axis=1)

    # ---- the shared proof ----
    def merkle4_forest_ragged_multiproof_bound(self, n_leaves, n_trees, max_leaves, k):
        return forest_multiproof_bound(n_leaves, n_trees, max_leaves, k, 4)

    def merkle2_forest_ragged_multiproof_bound(self, n_leaves, n_trees, max_leaves, k):
        return forest_multiproof_bound(n_leaves, n_trees, max_leaves, k, 2)

    def _mp(self, arity, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k, d_leaves_out, d_proof, d_proof_offsets, d_n_bad=None):
        sizes = good_leaf_counts(d_offsets, d_leaves.shape[0], max_leaves)
        off = TS.offsets(sizes, int(d_offsets[0])).astype(np.int64)
        out, proof, po = forest_multiproof_extract(d_leaves, off, d_levels, d_tree_ids[:k], d_leaf_ids[:k], arity)
        d_leaves_out[:k], d_proof_offsets[:] = out, po
        if proof.shape[0] <= (d_proof.shape[0] if d_proof is not None else 0):
            d_proof[:proof.shape[0]] = proof

    def merkle4_forest_ragged_multiproof_device(self, *args):
        self._mp(4, *args)

    def merkle2_forest_ragged_multiproof_device(self, *args):
        self._mp(2, *args)

    def _mp_verify(self, arity, tag, d_offsets, n_leaves, n_trees, max_leaves, d_tree_ids, d_leaf_ids, d_leaves_in, k, d_proof, proof_len, d_proof_offsets,
                   d_roots, d_ok, d_roots_out=None, d_n_hashed=None, d_n_bad=None):
        sizes = good_leaf_counts(d_offsets, n_leaves, max_leaves)
        digest = lambda ch: E.oracle.hash_batch(tag, E.reduce_mod_p(ch), arity, 1).reshape(-1, 4)  # noqa: E731
        proof = d_proof[:proof_len] if proof_len else np.zeros((0, 4), np.uint64)
        roots = forest_multiproof_roots(sizes, d_tree_ids[:k], d_leaf_ids[:k], d_leaves_in[:k], proof, d_proof_offsets, arity, digest, E.reduce_mod_p)
        d_ok[:] = 0
        for t, r in roots.items():
            if r is not None:
                d_ok[t] = np.array_equal(r, d_roots[t])
                if d_roots_out is not None:
                    d_roots_out[t] = r
        if d_n_hashed is not None:
            d_n_hashed[0] += forest_multiproof_counts(sizes, d_tree_ids[:k], d_leaf_ids[:k], arity)[1]

    def merkle4_forest_ragged_multiproof_verify_device(self, *args):
        self._mp_verify(4, *args)

    def merkle2_forest_ragged_multiproof_verify_device(self, *args):
        self._mp_verify(2, *args)


@pytest.mark.parametrize("arity", [4, 2])
def test_the_runner_passes_the_small_plans_on_the_stand_in(arity):
    had_torch = "torch" in sys.modules
    w = W.run(_plan("small", arity), HostBackend())
    assert had_torch or "torch" not in sys.modules  # the runner's only seam is dev / host
    assert len(w.fresh_only) == len(w.plan.steps) + 2 and not any(w.fresh_only)  # the build, every step, the final state: the oracle on every tree


# ---------------------------------------------------------------------------------------------- 4. the checks bite
def _first(P, kind, n):
    """the index of the n-th step of a kind (a resize: any call that goes to the resize entry point)"""
    kinds = RESIZES if kind == "resize" else (kind,)
    return [i for i, s in enumerate(P.steps, 1) if s["kind"] in kinds][n - 1]


@pytest.mark.parametrize("fault, kind, nth, says", [
    ("stale_top", "update", 2, "the levels differ from the oracle, first at \\(tree \\d+, level \\d+, node 0\\)"),
    ("copied", "resize", 1, "the levels differ from the oracle, first at \\(tree \\d+, level 1, node \\d+\\)"),
    ("raw_root", "append", 1, "the roots differ from the oracle, first at \\(tree 40, level 0, node 0\\)"),
    ("past_used", "update", 3, "the update wrote at or past the used length \\d+ of d_levels"),
], ids=["a-update-leaves-a-top-node-stale", "b-resize-copies-a-dirty-node", "c-append-writes-a-raw-one-leaf-root", "d-update-writes-past-the-used-levels"])
def test_a_stand_in_that_is_wrong_in_one_way_is_rejected_at_that_step(fault, kind, nth, says):
    P = _plan("small", 4)
    at = _first(P, kind, nth)
    with pytest.raises(AssertionError, match="^step %d \\(%s\\): %s" % (at, P.steps[at - 1]["kind"], says)):
        W.run(P, HostBackend(fault=(fault, nth)))
