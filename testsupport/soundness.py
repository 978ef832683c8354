"""Every single change to a good proof, and what a sound verifier answers: the catalogue that tests/test_soundness_gpu.py puts to the
five Merkle verifiers (p252_merkle{4,2}_multiproof_verify_device, _forest_ragged_multiproof_verify_device_into, _verify_batch_device,
_forest_ragged_verify_device, the latter also on anchored openings) and that tests/test_soundness_cpu.py checks against deliberately
wrong verifiers.  Numpy, treeshape and multiproofmodel alone: no torch, nothing of the library.

The expected verdict never comes from the code under test.  For the shared proofs it is multiproofmodel's multiproof_root /
forest_multiproof_roots; for the openings it is `rehash` below (the one numpy re-hash of an opening; tests/edgecases.py wraps it).  The
digest is a parameter, digest((m, arity, 4)) -> m scalars, and sees reduced scalars only (`reducing` wraps one so).

A case is (class name, changed inputs, expectation).  The expectation is the class's own structural claim — REFUSE, ACCEPT, UNWRITTEN
(refused and the root output left alone: the structure failed), SAME (the good input's verdict) or MODEL (no structural claim: what the
model says) — and the CPU test shows that the model agrees with it on every case.

The position byte: the four path / verify calls read its low two bits (arity 2: one bit) and nothing else, so `rehash` masks it."""
import numpy as np

from . import multiproofmodel as MM
from . import treeshape as TS

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # the scalar field's modulus (test_soundness_cpu: the oracle's)
M64 = (1 << 64) - 1
REFUSE, ACCEPT, UNWRITTEN, SAME, MODEL = "refuse", "accept", "unwritten", "same", "model"
NO_TREE = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- 256-bit scalars as four uint64 limbs
def _add_const(a, c):
    a = np.asarray(a, dtype=np.uint64)
    out, carry = np.empty_like(a), np.zeros(a.shape[:-1], dtype=np.uint64)
    for i in range(4):
        ci = np.uint64((c >> (64 * i)) & M64)
        s = a[..., i] + ci
        s2 = s + carry
        out[..., i] = s2
        carry = ((s < ci) | (s2 < carry)).astype(np.uint64)
    return out


def _below_p(a):
    lt, eq = np.zeros(a.shape[:-1], dtype=bool), np.ones(a.shape[:-1], dtype=bool)
    for i in (3, 2, 1, 0):
        pi = np.uint64((P >> (64 * i)) & M64)
        lt |= eq & (a[..., i] < pi)
        eq &= a[..., i] == pi
    return lt


def reduce_mod_p(a):
    """V mod p over (..., 4) limbs (V < 2^256 < 3p)"""
    a = np.array(a, dtype=np.uint64)
    for _ in range(2):
        a = np.where(_below_p(a)[..., None], a, _add_const(a, (1 << 256) - P))
    return a


def plus_p(a):
    """the limbs of V + p, for V < 2^256 - p"""
    return _add_const(a, P)


def reducing(digest):
    """digest as the models call it: inputs reduced first (a value that is hashed counts mod p), (m, 4) out"""
    def hashed(kids):
        kids = reduce_mod_p(kids)
        rows, back = np.unique(kids.reshape(kids.shape[0], -1), axis=0, return_inverse=True)  # (equal children: one digest)
        return np.asarray(digest(rows.reshape((-1,) + kids.shape[1:])), dtype=np.uint64).reshape(-1, 4)[back.reshape(-1)]
    return hashed


def flip(scalar, rng):
    """one random bit (0 .. 255) of the scalar, in place -> the bit"""
    b = int(rng.integers(0, 256))
    scalar[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return b


def index_sets(n, arity):
    """the position sets of the shared-proof tests"""
    last_pair = (n - 1) // arity * arity  # the last parent's first child; with its neighbour when the tree has one
    pair = [last_pair, last_pair + 1] if last_pair + 1 < n else [0, 1] if n > 1 else [0]
    return {"first": [0], "last": [n - 1], "ends": sorted({0, n - 1}), "one parent": pair, "every other": list(range(0, n, 2)),
            "all": list(range(n))}


# ---------------------------------------------------------------------------------------------- the re-hash of an opening
def children(cur, sib_level, pos_level, arity):
    """the node's children: the siblings in ascending slot order with `cur` inserted at its position"""
    n = cur.shape[0]
    ch = np.empty((n, arity, 4), dtype=np.uint64)
    rows = np.arange(n)
    for s in range(arity):
        si = np.minimum(np.where(s > pos_level, s - 1, s), arity - 2)
        ch[:, s] = np.where((pos_level == s)[:, None], cur, sib_level[rows, si])
    return ch


def rehash(digest, arity, leaves, sib, pos, depths=None):
    """roots of openings, level by level through digest((m, arity, 4)) (opening i stops after depths[i] levels); of a position byte the
    low bits below the arity count"""
    cur = np.array(leaves, dtype=np.uint64).reshape(-1, 4)
    n, depth = cur.shape[0], pos.shape[1]
    sib = np.asarray(sib, dtype=np.uint64).reshape(n, depth, arity - 1, 4)
    for l in range(depth):
        live = np.arange(n) if depths is None else np.nonzero(depths > l)[0]
        if live.size == 0:
            break
        ch = children(cur[live], sib[live, l], pos[live, l].astype(np.int64) & (arity - 1), arity)
        cur[live] = np.asarray(digest(ch), dtype=np.uint64).reshape(-1, 4)
    return cur


def open_tree(leaves, levels, arity, stride):
    """every leaf's opening out of a stored tree (levels bottom-up) at the stride `stride`, as p252_merkle{4,2}_forest_ragged_openings_device
    lays it out: (leaves (n, 4), siblings (n, stride, arity - 1, 4), positions (n, stride) uint8, depths (n,) uint8); missing siblings and
    the rows at or past the depth are zero"""
    per_level = MM._split_levels(leaves, levels, arity)
    n, d = per_level[0].shape[0], len(per_level) - 1
    assert d == TS.depth(n, arity) <= stride
    sib, pos = np.zeros((n, stride, arity - 1, 4), dtype=np.uint64), np.zeros((n, stride), dtype=np.uint8)
    node = np.arange(n)
    for l in range(d):
        pos[:, l] = node % arity
        for s in range(arity):
            c = node - node % arity + s
            there = (c != node) & (c < per_level[l].shape[0])
            slot = s - (s > node % arity)
            sib[there, l, slot[there]] = per_level[l][c[there]]
        node = node // arity
    return np.array(per_level[0], dtype=np.uint64), sib, pos, np.full(n, d, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- shared proof, one tree
LIES = ("proof_len + 1", "proof_len - 1", "n_leaves + 1", "n_leaves - 1")  # in a forest they move an offset: the next tree changes too
SHARED_CLASSES = ("flip proof", "flip leaf", "flip root", "proof + p", "leaf + p", "root + p", "swap proof", "swap leaves", "proof_len + 1",
                  "proof_len - 1", "position + 1", "position - 1", "n_leaves + 1", "n_leaves - 1")


def shared_good(leaves, levels, pos, root, arity, spare):
    """the verifier's inputs for the positions `pos` of a stored tree: n, pos, leaves (k, 4), buf = the proof and one spare scalar behind
    it, plen = the length claimed, n0 / plen0 = the true ones"""
    leaves = np.asarray(leaves, dtype=np.uint64).reshape(-1, 4)
    pos = np.asarray(pos, dtype=np.int64)
    proof = MM.multiproof_extract(leaves, levels, pos, arity).astype(np.uint64)
    n = leaves.shape[0]
    return dict(n=n, n0=n, pos=pos, leaves=leaves[pos].copy(), buf=np.concatenate([proof, np.asarray(spare, dtype=np.uint64).reshape(1, 4)]),
                plen=proof.shape[0], plen0=proof.shape[0], root=np.array(root, dtype=np.uint64))


def _copy(x, **changed):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in x.items()}
    out.update(changed)
    return out


def _plan(x, arity, rng, proof_at=None, in_range_only=False):
    """[(class, expectation, change)] of the good inputs x: change(c) makes the case out of a copy c of x"""
    n, k, plen = x["n"], len(x["pos"]), x["plen"]
    at = range(plen) if proof_at is None else proof_at
    plan = []

    def scalar(name, key, i, expectation, plus):
        def change(c):
            if plus:
                c[key][i] = plus_p(c[key][i])
            else:
                flip(c[key][i], rng)
        plan.append((name, expectation, change))

    def swap(name, key, i):
        def change(c):
            c[key][[i, i + 1]] = c[key][[i + 1, i]]
        plan.append((name, REFUSE, change))

    def put(name, expectation, key, value, i=None):
        def change(c):
            if i is None:
                c[key] = value
            else:
                c[key][i] = value
        plan.append((name, expectation, change))
    for j in at:
        scalar("flip proof", "buf", j, REFUSE, False)
    for j in at:
        scalar("proof + p", "buf", j, ACCEPT, True)
    pairs = [j for j in at if j + 1 < plen and not np.array_equal(x["buf"][j], x["buf"][j + 1])]
    if pairs:
        swap("swap proof", "buf", pairs[int(rng.integers(len(pairs)))])
    if proof_at is not None:
        return plan
    for i in range(k):
        scalar("flip leaf", "leaves", i, REFUSE, False)
    for i in range(k):
        scalar("leaf + p", "leaves", i, ACCEPT if n > 1 else MODEL, True)  # (the one leaf of a single tree IS its root, compared as bytes)
    scalar("flip root", "root", slice(None), REFUSE, False)
    scalar("root + p", "root", slice(None), REFUSE, True)
    if k >= 2:
        i = int(rng.integers(k - 1))
        assert not np.array_equal(x["leaves"][i], x["leaves"][i + 1])
        swap("swap leaves", "leaves", i)
    put("proof_len + 1", UNWRITTEN, "plen", plen + 1)
    if plen:
        put("proof_len - 1", UNWRITTEN, "plen", plen - 1)
    for d in (1, -1):
        for i in range(k):
            new = int(x["pos"][i]) + d
            if 0 <= new < n and (i == 0 or x["pos"][i - 1] < new) and (i == k - 1 or new < x["pos"][i + 1]):
                put("position %s 1" % "+-"[d < 0], MODEL, "pos", new, i)
    put("n_leaves + 1", MODEL, "n", n + 1)
    if n > 1 and not (in_range_only and int(x["pos"][-1]) == n - 1):
        put("n_leaves - 1", MODEL, "n", n - 1)
    return plan


def _made(x, entry):
    c = _copy(x)
    entry[2](c)
    return entry[0], c, entry[1]


def shared_cases(x, arity, rng, proof_at=None, in_range_only=False):
    """[(class, changed inputs, expectation)] of the good inputs x: every scalar the model reads gets its bit flip and its + p.  proof_at:
    only the flips, + p and swap of those proof scalars; in_range_only leaves out n_leaves - 1 where the last position is n - 1"""
    return [_made(x, e) for e in _plan(x, arity, rng, proof_at, in_range_only)]


def shared_one(x, arity, rng, skip=()):
    """one case of shared_cases, drawn evenly among those whose class is not in `skip`"""
    plan = [e for e in _plan(x, arity, rng) if e[0] not in skip]
    return _made(x, plan[int(rng.integers(len(plan)))])


def shared_case_count(n, pos, arity):
    """the number of cases shared_cases makes of the positions `pos` of a tree of n leaves, by class, from the shape alone"""
    pos = np.asarray(pos, dtype=np.int64)
    k, plen = pos.size, MM.multiproof_counts(n, pos, arity)[0]
    gaps = int((np.diff(pos) > 1).sum())
    up, down = gaps + int(pos[-1] < n - 1), gaps + int(pos[0] > 0)
    return {"flip proof": plen, "flip leaf": k, "flip root": 1, "proof + p": plen, "leaf + p": k, "root + p": 1, "swap proof": int(plen >= 2),
            "swap leaves": int(k >= 2), "proof_len + 1": 1, "proof_len - 1": int(plen >= 1), "position + 1": up, "position - 1": down,
            "n_leaves + 1": 1, "n_leaves - 1": int(n > 1)}


def _bad_positions(n, pos):
    pos = np.asarray(pos, dtype=np.int64)
    return int(((pos >= n) | (pos < 0) | np.concatenate([[False], np.diff(pos) <= 0])).sum())


def shared_verdict(x, arity, digest):
    """the model: (ok, root_out or None where the structure fails, n_hashed, n_bad) of p252_merkle{4,2}_multiproof_verify_device"""
    bad = _bad_positions(x["n"], x["pos"])
    if bad:
        return 0, None, 0, bad
    hashed = MM.multiproof_counts(x["n"], x["pos"], arity)[1]
    root = MM.multiproof_root(x["n"], x["pos"], x["leaves"], x["buf"][:x["plen"]], arity, reducing(digest))
    if root is None:
        return 0, None, hashed, 0
    return int(np.array_equal(root, x["root"])), np.asarray(root, dtype=np.uint64), hashed, 0


def expected_ok(expectation, good_ok=1):
    """what the class claims, or None for MODEL"""
    return {REFUSE: 0, UNWRITTEN: 0, ACCEPT: 1, SAME: good_ok, MODEL: None}[expectation]


# ---------------------------------------------------------------------------------------------- shared proof, a forest
def forest_of(trees):
    """the forest verifier's inputs of a list of single-tree inputs: tree t claims trees[t]["n"] leaves and the proof part
    [po[t], po[t] + trees[t]["plen"]), and HOLDS its true part — so a length that lies moves the next tree's start, as an offset does"""
    sizes = np.array([x["n"] for x in trees], dtype=np.int64)
    true = TS.offsets([x["plen0"] for x in trees], dtype=np.int64)
    po = true.copy()
    po[1:] = true[:-1] + np.array([x["plen"] for x in trees], dtype=np.int64)
    assert po[-1] == true[-1], "the last tree of a forest must not lie about its length"
    return dict(sizes=sizes, off=TS.offsets(sizes), tid=np.concatenate([np.full(len(x["pos"]), t, dtype=np.int64) for t, x in enumerate(trees)]),
                lid=np.concatenate([x["pos"] for x in trees]), leaves=np.concatenate([x["leaves"] for x in trees]),
                proof=np.concatenate([x["buf"][:x["plen0"]] for x in trees] + [np.zeros((0, 4), dtype=np.uint64)]), plen=int(true[-1]),
                po=po.astype(np.uint64), roots=np.array([x["root"] for x in trees], dtype=np.uint64))


def copies_forest(cases, spare):
    """copy 0 untouched (cases[0] is the good input), copy i carries case i; behind every copy that lies about a length or a leaf count
    stands `spare` (a good input of few positions), resized so that the forest's leaf offsets stay consistent -> (trees, the index of case
    i's tree)"""
    trees, where = [], []
    for cls, x, _ in cases:
        where.append(len(trees))
        trees.append(x)
        if cls in LIES:
            trees.append(_copy(spare, n=spare["n"] - (x["n"] - x["n0"])))
    trees.append(_copy(spare))
    return trees, np.array(where)


def forest_verdict(F, arity, digest):
    """the model: (ok (T,), roots_out: list of root or None per tree, n_hashed, n_bad) of
    p252_merkle{4,2}_forest_ragged_multiproof_verify_device_into, for pairs none of which is bad"""
    T, sizes = len(F["sizes"]), F["sizes"]
    assert (F["lid"] < sizes[F["tid"]]).all() and (F["lid"] >= 0).all()
    po = F["po"].astype(np.int64)
    roots = MM.forest_multiproof_roots(sizes, F["tid"], F["lid"], F["leaves"], F["proof"][:F["plen"]], po, arity, reducing(digest), reduce=reduce_mod_p)
    ok, out = np.zeros(T, dtype=np.uint8), [None] * T
    for t, r in roots.items():
        if r is not None and po[t] <= po[t + 1] <= F["plen"]:
            out[t] = np.asarray(r, dtype=np.uint64)
            ok[t] = np.array_equal(out[t], F["roots"][t])
    return ok, out, MM.forest_multiproof_counts(sizes, F["tid"], F["lid"], arity)[1], 0


# ---------------------------------------------------------------------------------------------- openings
def openings_good(parts, stride):
    """one batch of the openings of several trees: parts = [(leaves, siblings, positions, depths, root)] at the stride `stride` each ->
    dict(leaves, sib, pos, dep, tid, roots, stride)"""
    return dict(leaves=np.concatenate([p[0] for p in parts]), sib=np.concatenate([p[1] for p in parts]), pos=np.concatenate([p[2] for p in parts]),
                dep=np.concatenate([p[3] for p in parts]).astype(np.uint8), tid=np.concatenate([np.full(len(p[3]), t, dtype=np.uint32) for t, p in enumerate(parts)]),
                roots=np.array([p[4] for p in parts], dtype=np.uint64), stride=stride)


def opening_case_count(depths, stride, arity, ragged, n_trees):
    """rows of opening_cases per class, from the depths alone"""
    d = np.asarray(depths, dtype=np.int64)
    n, rows = d.size, int(d.sum())
    out = {"flip leaf": n, "flip sibling": rows * (arity - 1), "leaf + p": n, "sibling + p": rows * (arity - 1), "position other": rows * (arity - 1),
           "position + arity": rows, "position + 2 arity": rows, "position | 0x80": rows}
    if ragged:
        out.update({"flip past the depth": int((d < stride).sum()), "depth + 1": n, "depth - 1": int((d >= 1).sum()), "depth stride + 1": n,
                    "depth 0xFF": n, "tree id of another tree": n if n_trees > 1 else 0, "tree id n_trees": n, "tree id 0xFFFFFFFF": n})
    return out


def opening_cases(O, arity, rng, ragged):
    """every case of every opening of the good batch O as ONE batch: (batch, class per row, expectation per row, base opening per row).
    Row 0 .. n - 1 of the batch are the good openings themselves (class "good", ACCEPT).  ragged adds the depth byte, the tree id and the
    rows at or past the depth; a fixed-depth batch has neither."""
    n, D, A, T = len(O["dep"]), O["stride"], arity, len(O["roots"])
    base, cls, exp, todo = list(range(n)), ["good"] * n, [ACCEPT] * n, [None] * n

    def add(i, name, expectation, change):
        base.append(i), cls.append(name), exp.append(expectation), todo.append(change)
    for i in range(n):
        d = int(O["dep"][i])
        add(i, "flip leaf", REFUSE, ("flip", "leaves", ()))
        add(i, "leaf + p", ACCEPT, ("plus", "leaves", ()))
        for l in range(d):
            for s in range(A - 1):
                add(i, "flip sibling", REFUSE, ("flip", "sib", (l, s)))
                add(i, "sibling + p", ACCEPT, ("plus", "sib", (l, s)))
            p = int(O["pos"][i, l])
            for v in range(A):
                if v != p:
                    add(i, "position other", MODEL, ("set", "pos", (l,), v))
            add(i, "position + arity", SAME, ("set", "pos", (l,), p + A))
            add(i, "position + 2 arity", SAME, ("set", "pos", (l,), p + 2 * A))
            add(i, "position | 0x80", SAME, ("set", "pos", (l,), p | 0x80))
        if not ragged:
            continue
        if d < D:
            add(i, "flip past the depth", SAME, ("flip", "sib", (int(rng.integers(d, D)), int(rng.integers(A - 1)))))
        add(i, "depth + 1", REFUSE, ("set", "dep", (), d + 1))
        if d >= 1:
            add(i, "depth - 1", REFUSE if d > 1 else MODEL, ("set", "dep", (), d - 1))  # (depth 0 leaves the leaf as the "root")
        add(i, "depth stride + 1", REFUSE, ("set", "dep", (), D + 1))
        add(i, "depth 0xFF", REFUSE, ("set", "dep", (), 0xFF))
        t = int(O["tid"][i])
        others = [u for u in range(T) if not np.array_equal(O["roots"][u], O["roots"][t])]
        if T > 1:
            add(i, "tree id of another tree", REFUSE, ("set", "tid", (), others[int(rng.integers(len(others)))]))
        add(i, "tree id n_trees", REFUSE, ("set", "tid", (), T))
        add(i, "tree id 0xFFFFFFFF", REFUSE, ("set", "tid", (), NO_TREE))
    rows = np.asarray(base)
    B = dict(O, leaves=O["leaves"][rows].copy(), sib=O["sib"][rows].copy(), pos=O["pos"][rows].copy(), dep=O["dep"][rows].copy(), tid=O["tid"][rows].copy())
    for r, change in enumerate(todo):
        if change is None:
            continue
        target = B[change[1]][r]
        if change[0] == "set":
            B[change[1]][(r,) + change[2]] = change[3]
        elif change[0] == "flip":
            flip(target[change[2]], rng)
        else:
            target[change[2]] = plus_p(target[change[2]])
    return B, np.asarray(cls), np.asarray(exp), rows


def root_cases(O, rng):
    """[(class, the roots with EVERY root changed)]: against them no opening of the good batch verifies"""
    flipped = O["roots"].copy()
    for r in flipped:
        flip(r, rng)
    return [("flip root", flipped), ("root + p", plus_p(O["roots"]))]


def openings_verdict(B, arity, digest):
    """the model: ok (n,) of p252_merkle{4,2}_forest_ragged_verify_device — and of _verify_batch_device, whose batch has one tree and
    every depth at the stride"""
    dep, tid, T = B["dep"].astype(np.int64), B["tid"].astype(np.int64), len(B["roots"])
    formed = (dep <= B["stride"]) & (tid < T)
    got = rehash(reducing(digest), arity, reduce_mod_p(B["leaves"]), B["sib"], B["pos"], np.where(formed, dep, 0))
    return (formed & (got == B["roots"][np.where(formed, tid, 0)]).all(axis=1)).astype(np.uint8)


def expected_rows(exp, good_ok):
    """the classes' claims per row: 0 / 1, or -1 where the class leaves it to the model"""
    exp = np.asarray(exp)
    return np.where(exp == REFUSE, 0, np.where(exp == ACCEPT, 1, np.where(exp == SAME, good_ok, -1))).astype(np.int64)
