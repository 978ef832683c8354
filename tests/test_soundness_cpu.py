"""The soundness sweep without a GPU (testsupport/soundness.py, tests/soundcases.py): (a) on every case of every shape that
tests/test_soundness_gpu.py runs, the structural claim of the case's class equals the model's verdict — no case is skipped, no share of
disagreements tolerated — every class applies, and the case counts are those the shapes give; (b) the catalogue catches deliberately
wrong verifiers written here in Python, each by the classes named next to it, so a class taken out of the catalogue fails this file."""
import os
import re

import numpy as np
import pytest

import edgecases as E
import soundcases as C
from testsupport import soundness as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_catalogue_asks_neither_torch_nor_the_library_and_knows_the_oracles_modulus(oracle_mod):
    src = open(os.path.join(ROOT, "testsupport", "soundness.py")).read()
    assert set(re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", src, re.M)) == {"numpy", "."}
    assert set(re.findall(r"^from \. import (\w+)", src, re.M)) == {"multiproofmodel", "treeshape"}
    assert S.P == oracle_mod.P == E.P
    raw, red = E.edge_scalars(0x50, 300)
    assert np.array_equal(S.reduce_mod_p(raw), red) and np.array_equal(S.plus_p(red), E.plus_p(red))
    assert np.array_equal(S.reduce_mod_p(S.plus_p(red)), red)


# ---------------------------------------------------------------------------------------------- (a) the claims are the model's verdicts
def _claims_hold(cases, verdicts, what):
    """the good input verifies; every class's claim is the model's verdict; a failed structure leaves no root; a moved position is
    always refused"""
    assert cases[0][0] == "good" and verdicts[0][0] == 1 and np.array_equal(verdicts[0][1], cases[0][1]["root"])
    for (cls, x, expectation), v in zip(cases, verdicts):
        claim = S.expected_ok(expectation)
        assert claim is None or v[0] == claim, (what, cls, v)
        assert expectation != S.UNWRITTEN or v[1] is None, (what, cls)
        if cls.startswith("position"):
            assert v[0] == 0, (what, cls)
        if cls == "leaf + p" and x["n"] == 1:
            assert v[0] == 0  # (the one leaf of a single tree is its root, compared as the bytes it is)


@pytest.mark.parametrize("arity", [4, 2])
def test_shared_proof_of_one_tree(oracle_mod, arity):
    """cases per tree size, summed over the six position sets (soundness.shared_case_count: 2 (k + len) + 4 + [len >= 2] + [k >= 2] +
    [len >= 1] + the positions that can move up and down + [n > 1]):
    arity 4, n = 1, 2, 4, 5, 16, 17, 21, 64, 65: 36, 63, 100, 106, 191, 184, 209, 461, 442 — 1,792 in all;
    arity 2, n = 1, 2, 3, 7, 8, 9, 33: 36, 63, 81, 115, 124, 126, 258 — 803 in all"""
    per_n = {4: (36, 63, 100, 106, 191, 184, 209, 461, 442), 2: (36, 63, 81, 115, 124, 126, 258)}[arity]
    seen = set()
    for n, want in zip(C.SHARED_SHAPES[arity], per_n):
        total = 0
        for name, x, cases, verdicts in C.shared_single(arity, n):
            _claims_hold(cases, verdicts, (arity, n, name))
            counts = S.shared_case_count(n, x["pos"], arity)
            assert {c: sum(cls == c for cls, _, _ in cases) for c in S.SHARED_CLASSES} == counts, (arity, n, name)
            seen |= {c for c, k in counts.items() if k}
            total += len(cases) - 1
        assert total == want, (arity, n, total)
    assert seen == set(S.SHARED_CLASSES)


def test_scan_tile_borders(oracle_mod):
    """arity 4: 8 proof scalars next to a border or last, 17 cases (8 flips, 8 + p, a swap); arity 2: 3 scalars, 7 cases"""
    for arity, scalars, n_cases in ((4, 8, 17), (2, 3, 7)):
        x, at, cases, verdicts = C.shared_tiles(arity)
        assert len(at) == scalars and len(cases) - 1 == n_cases and at[-1] == x["plen"] - 1
        _claims_hold(cases, verdicts, ("tiles", arity))
        assert {c[0] for c in cases[1:]} == {"flip proof", "proof + p", "swap proof"}


@pytest.mark.parametrize("arity,n,n_cases,n_trees", [(4, 21, 205, 231), (4, 65, 438, 464), (2, 9, 122, 148), (2, 33, 254, 280)])
def test_forest_of_copies(oracle_mod, arity, n, n_cases, n_trees):
    """the single-tree cases of the six position sets, less n_leaves - 1 where the last leaf is asked for (four sets), one copy each and
    six untouched ones; behind each copy that moves an offset an untouched copy, and one at the end"""
    F, where, cases, (ok, roots, hashed, bad) = C.shared_copies(arity, n)
    assert sum(c[0] != "good" for c in cases) == n_cases == sum(sum(S.shared_case_count(n, p, arity).values()) for p in S.index_sets(n, arity).values()) - 4
    assert len(F["sizes"]) == n_trees == len(cases) + sum(c[0] in S.LIES for c in cases) + 1 and bad == 0
    assert {c[0] for c in cases} == set(S.SHARED_CLASSES) | {"good"}
    for i, (cls, x, expectation) in enumerate(cases):
        claim, t = S.expected_ok(expectation), where[i]
        assert claim is None or ok[t] == claim, (cls, t)
        assert expectation != S.UNWRITTEN or roots[t] is None, cls
        if cls.startswith("position"):
            assert ok[t] == 0
        if cls in ("proof_len + 1", "proof_len - 1"):
            assert ok[t + 1] == 0 and roots[t + 1] is None  # (the copy behind it starts where the lie ends)
    assert ok[-1] == 1


def test_many_forest(oracle_mod):
    """3,000 trees, one case each (3,000 cases), then one in every third (1,000 cases): a tree left alone verifies"""
    for every, n_cases in ((1, 3000), (3, 1000)):
        F, classes, (ok, roots, hashed, bad) = C.shared_many(every)
        assert sum(c is not None for c in classes) == n_cases and not set(classes) & set(S.LIES)
        claims = {"flip proof": 0, "flip leaf": 0, "flip root": 0, "root + p": 0, "swap proof": 0, "swap leaves": 0, "position + 1": 0, "position - 1": 0,
                  "proof + p": 1, "leaf + p": 1, None: 1}
        assert set(classes) | {None} == set(claims)
        for t, cls in enumerate(classes):
            assert ok[t] == claims[cls], (every, t, cls)


def _rows_hold(sw, arity, ragged, what):
    claim = S.expected_rows(sw["exp"], 1)
    said = claim >= 0
    assert np.array_equal(sw["ok"][said], claim[said]), (what, set(sw["cls"][said][sw["ok"][said] != claim[said]]))
    good = sw["good"]
    counts = S.opening_case_count(good["dep"], good["stride"], arity, ragged, len(good["roots"]))
    assert {c: int((sw["cls"] == c).sum()) for c in counts} == counts and all(counts.values()), what
    assert len(sw["ok"]) == len(good["dep"]) + sum(counts.values())
    for cls, _, ok in sw["roots"]:
        assert not ok.any(), (what, cls)
    return sum(counts.values())


def test_openings_of_fixed_depth(oracle_mod):
    """per opening of depth d: 2 (1 + d (A - 1)) flips and + p, d (A - 1) other positions, 3 d high position bits — arity 4, trees of 64,
    21, 256, 65 leaves: 2,432 + 798 + 12,800 + 3,250 rows; arity 2, trees of 8, 16, 9, 33: 160 + 416 + 234 + 1,254; and two changed roots each"""
    want = {4: (2432, 798, 12800, 3250), 2: (160, 416, 234, 1254)}
    for arity in (4, 2):
        for (depth, n), rows in zip(C.FIXED_TREES[arity], want[arity]):
            assert _rows_hold(C.fixed_openings(arity, depth, n), arity, False, (arity, n)) == rows == n * (2 + 3 * depth * (arity - 1) + 3 * depth)


def test_ragged_and_anchored_openings(oracle_mod):
    """the fixed-depth rows of every opening at its own depth, and per opening a flip past the depth (where the depth is below the stride),
    four depth bytes (three at depth 0) and three tree ids: 91,906 rows (arity 4, 1,216 openings) and 83,652 (arity 2, 1,176 openings) of the
    mixed forest; 10,735 (243 openings under 16 anchors) and 2,796 (79 openings under 14 anchors) of the anchored one"""
    for make, want in ((C.ragged_openings, {4: (1216, 91906), 2: (1176, 83652)}), (C.anchored_openings, {4: (243, 10735), 2: (79, 2796)})):
        for arity in (4, 2):
            sw = make(arity)
            assert (len(sw["good"]["dep"]), _rows_hold(sw, arity, True, (make.__name__, arity))) == want[arity]
            one_level = (sw["cls"] == "depth - 1") & (sw["good"]["dep"][sw["rows"]] == 1)
            assert one_level.any() and not sw["ok"][one_level].any()  # (a leaf is not the root of its two-leaf tree)


# ---------------------------------------------------------------------------------------------- (b) wrong verifiers are caught
def _wrong_shared(x, arity, flaw):
    """a verifier of the shared proof that walks the proof as a stream -> (ok, root_out or None); flaw None: a sound one"""
    n, plen, digest = x["n"], x["plen"], S.reducing(C.digest(arity))
    if S._bad_positions(n, x["pos"]):
        return 0, None
    known, at, w = {int(p): v for p, v in zip(x["pos"], x["leaves"])}, 0, n
    while w > 1:
        up = {}
        for parent in sorted({c // arity for c in known}):
            kids = np.zeros((1, arity, 4), dtype=np.uint64)
            for s in range(arity):
                c = parent * arity + s
                if c in known:
                    kids[0, s] = known[c]
                elif c < w:
                    if at < (len(x["buf"]) if flaw == "no length check" else plen):
                        kids[0, s] = x["buf"][at]
                    at += 1
            up[parent] = digest(kids)[0]
        known, w = up, (w + arity - 1) // arity
    whole = {None: at == plen, "no length check": True, "reads past the length are zero": at >= plen}[flaw]
    if not whole:
        return 0, None
    return int(np.array_equal(known[0], x["root"])), known[0]


def _wrong_openings(B, arity, flaw):
    """a verifier of openings -> ok (n,); flaw None: a sound one"""
    digest, D, T = S.reducing(C.digest(arity)), B["stride"], len(B["roots"])
    dep, tid = B["dep"].astype(np.int64), B["tid"].astype(np.int64)
    if flaw == "depth clamped to the stride":
        dep = np.minimum(dep, D)
    formed = dep <= D
    if flaw != "tree id ignored":
        formed &= tid < T
    pos = B["pos"].astype(np.int64) if flaw == "position compared whole" else B["pos"].astype(np.int64) & (arity - 1)
    sib = B["sib"].copy()
    if flaw == "zero padding skipped":  # a slot whose low limb is zero is taken for padding and not read further
        sib[sib[..., 0] == 0] = 0
    cur = S.reduce_mod_p(B["leaves"])
    for l in range(D):
        live = np.nonzero(formed & (dep > l))[0]
        level = sib[live, l]
        if flaw == "sibling index off by one at the last position":
            last = pos[live, l] == arity - 1
            level[last] = np.roll(level[last], 1, axis=1)
        cur[live] = digest(S.children(cur[live], level, pos[live, l], arity))
    limbs = 3 if flaw == "root compared on three limbs" else 4
    if flaw == "tree id ignored":
        same = (cur[:, None, :] == B["roots"][None, :, :]).all(axis=2).any(axis=1)
    else:
        same = (cur[:, :limbs] == B["roots"][np.where(formed, tid, 0)][:, :limbs]).all(axis=1)
    return (formed & same).astype(np.uint8)


SHARED_MUTANTS = {"no length check": {"proof_len + 1", "proof_len - 1"}, "reads past the length are zero": {"proof_len - 1"}}
OPENING_MUTANTS = {"tree id ignored": {"tree id n_trees", "tree id 0xFFFFFFFF"}, "zero padding skipped": {"flip sibling"},
                   "root compared on three limbs": {"flip root"}, "sibling index off by one at the last position": {"good", "leaf + p", "position + arity"},
                   "depth clamped to the stride": {"depth stride + 1", "depth 0xFF"}, "position compared whole": {"position + arity", "position + 2 arity", "position | 0x80"}}


def test_wrong_shared_proof_verifiers_are_caught(oracle_mod):
    """no length check; reads past proof_len give zero and a short proof passes for whole (the latter shows only in root_out, which a
    refused structure must leave alone)"""
    sweeps = [s for n in (5, 21) for s in C.shared_single(4, n)]
    for flaw in (None,) + tuple(SHARED_MUTANTS):
        caught = set()
        for name, _, cases, verdicts in sweeps:
            for (cls, x, _), want in zip(cases, verdicts):
                ok, root = _wrong_shared(x, 4, flaw)
                if ok != want[0] or (root is None) != (want[1] is None) or (root is not None and not np.array_equal(root, want[1])):
                    caught.add(cls)
        assert caught >= SHARED_MUTANTS[flaw] if flaw else not caught, (flaw, caught)


def test_wrong_opening_verifiers_are_caught(oracle_mod):
    """the tree id ignored; the zero padding slot skipped; the root compared on three limbs; the sibling index off by one at position
    arity - 1; the depth byte clamped to the stride; the position byte compared whole where the header says it is masked (the other half of
    that mistake, masking where forest_consistency_verify compares the whole byte, is test_forest_consistency_gpu's sweep to catch)"""
    sw = C.anchored_openings(4)
    B, O = sw["batch"], sw["good"]
    for flaw in (None,) + tuple(OPENING_MUTANTS):
        differs = _wrong_openings(B, 4, flaw) != sw["ok"]
        caught = set(sw["cls"][differs])
        for cls, roots, want in sw["roots"]:
            if not np.array_equal(_wrong_openings(dict(O, roots=roots), 4, flaw), want):
                caught.add(cls)
        assert caught >= OPENING_MUTANTS[flaw] if flaw else not caught, (flaw, caught)
