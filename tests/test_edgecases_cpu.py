"""The edge-value matrix's own ground, on the CPU alone: the generator of tests/edgecases.py meets its coverage condition, the
oracle, the big-int model and the host build of the device arithmetic agree on EVERY pattern (the host build on the raw,
unreduced words), and every hashing kernel of csrc/*.hip is named by a row of the matrix."""
import ctypes

import numpy as np
import pytest

import edgecases as E
import pymodel

P = pymodel.P
RINV = pow(1 << 256, -1, P)
u64p = ctypes.POINTER(ctypes.c_uint64)


def p(a):
    return a.ctypes.data_as(u64p)


def _ints(a):
    return [sum(int(v[i]) << (64 * i) for i in range(4)) for v in np.asarray(a).reshape(-1, 4)]


def _canon(a):
    """Montgomery limbs -> the values the big-int model works on"""
    return [v * RINV % P for v in _ints(a)]


@pytest.fixture(scope="module")
def perm():
    C, M = pymodel.load_constants()
    return lambda x: pymodel.perm_reference(x, C, M)


def _states():
    """every pattern in every one of the five positions (the other four walk through the patterns too), and all-equal states"""
    n = len(E.PATTERNS)
    rows = [[E.PATTERNS[(k + 7 * ((j - pos) % 5)) % n] for j in range(5)] for pos in range(5) for k in range(n)]
    rows += [[v] * 5 for v in E.PATTERNS]
    for pos in range(5):
        assert {r[pos] for r in rows} == set(E.PATTERNS)
    return rows


def _limbs(rows, reduce):
    return np.array([[E.limbs(v % P if reduce else v) for v in r] for r in rows], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------- the generator
def test_patterns_hold_what_the_issue_lists():
    pats = set(E.PATTERNS)
    assert len(pats) == len(E.PATTERNS)
    R = (1 << 256) % P
    d29 = (1 << 29) - 1
    for v in [0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, (1 << 256) - 1, (1 << 256) - (1 << 32), 1 << 255, 1 << 254,
              (P - 1) // 2, P * (((1 << 256) - 1) // P), R, R * R % P, P - R, int("55" * 32, 16), int("aa" * 32, 16)]:
        assert v in pats, hex(v)
    assert P * (((1 << 256) - 1) // P) + P >= 1 << 256
    for i in range(9):
        for v in (1 << (29 * i), (1 << (29 * i)) - 1, d29 << (29 * i)):
            assert v & ((1 << 256) - 1) in pats
    for i in range(1, 8):
        assert 1 << (32 * i) in pats and (1 << (32 * i)) - 1 in pats
    assert 3 * sum(v >= P for v in E.PATTERNS) < len(E.PATTERNS)  # (why the generator draws the patterns >= p apart)


@pytest.mark.parametrize("shape", [(9, 4), (300, 5), (8193, 5), (16385, 4), (64, 4), (100,), (8193, 8)])
def test_generator_contract(oracle_mod, shape):
    raw, red, index = E.edge_draw(77, shape)
    assert raw.shape == shape + (4,) == red.shape and raw.dtype == red.dtype == np.uint64
    again = E.edge_scalars(77, shape)
    assert np.array_equal(again[0], raw) and np.array_equal(again[1], red)  # seeded
    assert not np.array_equal(E.edge_scalars(78, shape)[0], raw)
    r, d = _ints(raw), _ints(red)
    assert all(a % P == b and b < P for a, b in zip(r, d))  # raw = reduced (mod p), reduced < p
    flat = index.reshape(-1)
    n_pat = int((flat >= 0).sum())
    assert abs(2 * n_pat - flat.size) <= 1  # about half are patterns
    assert all(E.PATTERNS[k] == v for k, v in zip(flat, r) if k >= 0)
    assert 3 * sum(E.PATTERNS[k] >= P for k in flat if k >= 0) >= n_pat  # at least a third of them with limbs >= p
    assert E.is_reduced(red).all() and np.array_equal(E.reduce_mod_p(raw), red)
    # patterns are not laid out in blocks: no run of equal neighbours longer than chance allows
    same = (flat[1:] == flat[:-1]) & (flat[1:] >= 0)
    assert same.sum() <= 4 + flat.size // len(E.PATTERNS)


@pytest.mark.parametrize("seed,shape", [(0x1000 + 16385, (16385, 4)), (0x1000 + 131073, (131073, 4)), (0x1000 + 8193, (8193, 4)),
                                        (0x3000 + 8193, (8193, 5))])
def test_every_pattern_at_every_position(oracle_mod, seed, shape):
    """the draws of the digest and permutation rows (their seeds and sizes): every entry of PATTERNS occurs at every state
    position — the columns 1..4 of a digest's state, all five of a permutation's (position 0 is where a sponge holds its tag)"""
    _, _, index = E.edge_draw(seed, shape)
    everything = set(range(len(E.PATTERNS)))
    for col in range(shape[1]):
        assert set(index[:, col].tolist()) >= everything, col
    for n in (300, 64):  # the lane-group rows: every pattern occurs in the batch
        _, _, small = E.edge_draw(seed, (n, 9))
        assert set(small.reshape(-1).tolist()) >= everything


def test_vectorised_arithmetic_matches_big_ints_and_the_oracle(oracle_mod):
    vals = sorted({(v + d) & E.M256 for v in E.PATTERNS for d in (-1, 0, 1)})
    a = np.array([E.limbs(v) for v in vals], dtype=np.uint64)
    lib = oracle_mod.lib()
    assert [bool(lib.p252o_is_reduced(p(np.ascontiguousarray(x)))) for x in a] == [v < P for v in vals] == E.is_reduced(a).tolist()
    assert _ints(E.reduce_mod_p(a)) == [v % P for v in vals]
    canon = np.array([E.limbs(v) for v in vals if v < P], dtype=np.uint64)
    twin = _ints(E.unreduced_twin(canon))
    for x, t in zip(_ints(canon), twin):
        assert t % P == x and t >= P and t < 1 << 256 and (t == x + 2 * P or x + 2 * P >= 1 << 256)
    assert _ints(E.plus_p(canon)) == [x + P for x in _ints(canon)]


@pytest.mark.parametrize("arity", [4, 2])
def test_level_by_level_references_match_the_oracles_own_calls(oracle_mod, arity):
    """the rows build large trees and re-hash openings level by level through the threaded oracle.hash_batch: the same scalars
    as oracle.merkle{4,2}_tree and oracle.merkle4_path_batch give"""
    tag = oracle_mod.tag(0, [4], 1) if arity == 4 else oracle_mod.tag(1, [2], 1)
    tree = oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree
    for n in (1, 2, arity, arity + 1, 341):
        _, red = E.edge_scalars(n, (n,))
        root, levels = E.oracle_tree(tag, red, arity)
        o_root, o_levels, _ = tree(tag, red, want_levels=True)
        assert np.array_equal(root, o_root) and np.array_equal(levels, o_levels), n
    if arity == 4:
        n, depth = 64, 5
        _, red = E.edge_scalars(9, (n, 1 + 3 * depth))
        pos = np.random.default_rng(9).integers(0, 4, size=(n, depth), dtype=np.uint8)
        sib = red[:, 1:].reshape(n, depth, 3, 4)
        assert np.array_equal(E.rehash(tag, 4, red[:, 0], sib, pos), oracle_mod.merkle4_path_batch(tag, red[:, 0], sib, pos))
        depths = np.arange(n) % (depth + 1)
        short = E.rehash(tag, 4, red[:, 0], sib, pos, depths)
        for i in range(n):
            assert np.array_equal(short[i], oracle_mod.merkle4_path_batch(tag, red[i:i + 1, 0], sib[i:i + 1, :depths[i]], pos[i:i + 1, :depths[i]])[0])


# ---------------------------------------------------------------------------------------------- oracle against big-int model
def test_oracle_permutation_matches_the_model_on_every_pattern(oracle_mod, perm):
    rows = _states()
    st = _limbs(rows, reduce=True)
    out = oracle_mod.permute_batch(st)
    assert E.is_reduced(out).all()
    for s, o in zip(st, out):
        assert _canon(o) == perm(_canon(s))


@pytest.mark.parametrize("in_len,out_len", [(1, 1), (4, 1), (2, 1), (5, 2), (9, 6)])
def test_oracle_sponge_matches_the_model_on_edge_messages(oracle_mod, perm, in_len, out_len):
    n = len(E.PATTERNS)
    _, red, index = E.edge_draw(100 * in_len + out_len, (n, in_len))
    for k in range(n):  # every pattern as a message element, at a position that moves through the message
        red[k, k % in_len] = E.limbs(E.PATTERNS[k] % P)
    tags = [oracle_mod.tag(3, [in_len], out_len)] + [E.limbs(v % P) for v in E.PATTERNS]  # the domain's tag, and every pattern as a tag
    for t, tag in enumerate(tags):
        rows = red if t == 0 else red[(t - 1) % n:(t - 1) % n + 1]
        got = oracle_mod.hash_batch(tag, rows, in_len, out_len)
        for m, g in zip(rows, got):
            assert _canon(g) == pymodel.sponge(_canon(tag)[0], _canon(m), out_len, perm=perm)


# ---------------------------------------------------------------------------------------------- the host build, on RAW words
def test_host_build_hashes_raw_patterns_as_their_residues(oracle_mod, hosttest_lib, perm):
    """csrc/fr29.hpp + hades29.hpp compiled for the host, all three schedules, fed the UNREDUCED patterns: the permutation of
    V mod p, canonical outputs — and the digest path with the hoisted tag S-box (k_merkle4's specialisation) likewise"""
    rows = _states()
    raw, red = _limbs(rows, reduce=False), _limbs(rows, reduce=True)
    want = oracle_mod.permute_batch(red)
    for s, o in list(zip(red, want))[::37]:  # (the oracle itself: checked in full above)
        assert _canon(o) == perm(_canon(s))
    for sched in (0, 1, 2):
        out = np.empty_like(raw)
        hosttest_lib.ht_permute29_sched(p(raw), p(out), raw.shape[0], sched)
        assert np.array_equal(out, want), "schedule %d" % sched
    # the digest path: children = positions 1..4 of the same states, the tag = each state's position 0 — raw against reduced
    n = raw.shape[0]
    for k in range(0, n, max(1, n // len(E.PATTERNS))):
        tag_raw, tag_red = np.ascontiguousarray(raw[k, 0]), np.ascontiguousarray(red[k, 0])
        x_raw, x_red = np.ascontiguousarray(raw[:, 1:]), np.ascontiguousarray(red[:, 1:])
        lo = k - k % 64
        a = np.empty((64, 4), dtype=np.uint64)
        m = min(64, n - lo)
        hosttest_lib.ht_merkle4_digest29(p(tag_raw), p(x_raw[lo:lo + m]), p(a), m)
        assert np.array_equal(a[:m], oracle_mod.hash_batch(tag_red, x_red[lo:lo + m], 4, 1).reshape(m, 4)), k


# ---------------------------------------------------------------------------------------------- the matrix names every kernel
def test_every_hashing_kernel_is_named_by_a_row():
    kernels = E.hashing_kernels()
    assert {"k_permute", "k_merkle4", "k_merkle4_pad", "k_merkle4_coop", "k_sponge_lines_trunc", "k_crypt_coop", "k_fr_digest",
            "k_fu_digest_coop", "k_mp_digest", "k_path_ragged", "k_merkle2_path", "k_sponge_ragged_coop_trunc"} <= kernels  # (the parser sees them)
    assert not any(k.startswith("k_pt_") for k in kernels) and "k_to_canonical" not in kernels and "k_fr_prep" not in kernels
    missing = kernels - E.named_kernels()
    assert not missing, "hashing kernels that no row of the edge matrix names: %s" % sorted(missing)
    assert len({r.name for r in E.ROWS}) == len(E.ROWS)
    for env, names, reached in E.CHILDREN.values():
        assert names and reached and all(n in E.BY_NAME for n in names)


def test_kernel_names_match_traced_names():
    traced = ["void p252::k_merkle4_coop<8>(int const*, p252::TagArg, p252::Scalar32 const*)", "p252::k_merkle4_lat(int const*)",
              "_ZN4p2529k_merkle4EPKiNS_6TagArgE", "p252::k_crypt<true>(int const*) [clone .kd]"]
    assert E.kernel_in_trace("k_merkle4_coop", traced) and E.kernel_in_trace("k_merkle4_lat", traced) and E.kernel_in_trace("k_merkle4", traced)
    assert E.kernel_in_trace("k_crypt", traced) and not E.kernel_in_trace("k_crypt_coop", traced)
    assert not E.kernel_in_trace("k_merkle4", traced[:2]) and not E.kernel_in_trace("k_merkle4_trunc", traced)
