"""The shape lists of tests/shapecases.py, without a GPU: that they reach every class of the kernels' shape-dependent branching (proved
against the dispatch model, as EQUALITIES with the class sets written out here: a list that shrinks fails), that the model's
cipher walk is the state machine the big-integer sponge runs, and that the oracle is right at every shape the sweep compares the
kernels with (against the big-integer restatements of tests/pymodel.py)."""
import itertools
import os

import numpy as np
import pytest

import pymodel
import shapecases as S

STREAM, DUPLEX = S.STREAM, S.DUPLEX
# (out_len mod 4, squeeze blocks) of out_len 1 .. 9: a partial and a full block, alone and after a full one, and a third block
OUT_CLASSES = {(1, 1), (2, 1), (3, 1), (0, 1), (1, 2), (2, 2), (3, 2), (0, 2), (1, 3)}
# one absorb block, one squeeze block of one scalar: in_len 4 or 2 with out_len 1 — the shapes that go to the digest kernels
DIGEST_OUT = (1, 1)


def _lanes(n):
    return range(n)


# ---------------------------------------------------------------------------------------------- the sponge
def _sponge_classes(n, coop_max, line_fetch):
    """{kernel: the classes its lanes fall in} over the whole sweep at n"""
    seen = {}
    for (in_len, out_len), offset, truncated in itertools.product(S.SPONGE_SHAPES, S.SPONGE_LAYOUTS, (False, True)):
        kernel = S.sponge_kernel(n, in_len, out_len, offset, truncated, coop_max, line_fetch)
        lines = "lines" in kernel
        for idx in _lanes(n):
            seen.setdefault(kernel, set()).add(S.sponge_class(in_len, out_len, offset, idx, lines))
    return seen


def test_excluded_shapes_are_the_digest_kernels():
    """(4, 1) and (2, 1) are not in the list: hash_batch_device hands them to the single-permutation digest kernels (api.cpp
    hash_batch_device_impl), so no sponge kernel ever sees them — the digest rows of tests/edgecases.py cover them"""
    assert S.DIGEST_SHAPES == ((4, 1), (2, 1))
    assert not set(S.DIGEST_SHAPES) & set(S.SPONGE_SHAPES)
    api = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "poseidon252_amd", "csrc", "api.cpp")).read()
    body = api[api.index("static int hash_batch_device_impl"):api.index("int p252_hash_batch_device(")]
    assert "in_len == 4 && out_len == 1" in body and "in_len == 2 && out_len == 1" in body and body.count("launch_merkle4(") == 2
    assert body.count("launch_sponge(") == 1
    with pytest.raises(AssertionError):
        S.sponge_kernel(323, 4, 1, 0, False)


def test_the_sponge_list_is_the_one_the_issue_sets():
    want = {(i, o) for i in range(1, 19) for o in range(1, 10)} | {(i, o) for i in (40, 41, 42, 43, 44) for o in (1, 4, 5, 8)}
    assert set(S.SPONGE_SHAPES) == want - {(4, 1), (2, 1)} and len(S.SPONGE_SHAPES) == len(set(S.SPONGE_SHAPES)) == 180
    assert S.SPONGE_LAYOUTS == (0, 32, 64) and S.RAGGED_IN_LENS == tuple(range(1, 19))
    assert S.CRYPT_LENS == tuple(range(1, 19)) + (41, 42, 43) and len(S.CRYPT_CASES) == 42
    assert S.PATH_DEPTHS == tuple(range(14)) + (16, 20) and len(S.PATH_CASES) == 32
    assert (S.N_LANE_GROUPS, S.N_ONE_LANE) == (70, 323)
    assert S.coop8(70) and S.coop8(8192) and not S.coop8(8193) and not S.coop8(70, 0) and not S.coop8(20000, 1 << 20)


def test_whole_line_sponge_classes_are_all_reached():
    """every reachable (in_len mod 4, line phase, absorb blocks, tail_half, trip of `parked`) x (out_len mod 4, squeeze blocks) of
    sponge_body<true>, for the plain and the truncating build.  tail_half and `parked` follow from the first three: a message ends
    in mid-line when (phase + in_len) mod 4 = 2, and its last fetch is its first when it has one block."""
    heads = {(0, 0, 1, False, None), (0, 0, 2, False, None), (0, 0, 3, False, None),
             (0, 2, 1, True, "first"), (0, 2, 2, True, "later"), (0, 2, 3, True, "later"),
             (2, 0, 1, True, "first"), (2, 0, 2, True, "later"), (2, 0, 3, True, "later"),
             (2, 2, 1, False, None), (2, 2, 2, False, None), (2, 2, 3, False, None)}
    want = {h + o for h in heads for o in OUT_CLASSES} - {h + DIGEST_OUT for h in heads if h[2] == 1}
    assert len(want) == 12 * 9 - 4
    seen = _sponge_classes(S.N_ONE_LANE, 0, True)
    assert seen["k_sponge_lines"] == want
    assert seen["k_sponge_lines_trunc"] == want
    assert {c[3] for c in want} == {True, False} and {c[4] for c in want} == {None, "first", "later"}


def test_block_by_block_sponge_classes_are_all_reached():
    """every reachable (in_len mod 4, absorb blocks) x (out_len mod 4, squeeze blocks) of sponge_body<false>: with whole lines (the odd
    lengths and the layout at +32 B) and without (P252_LINE_FETCH=0: every layout), plain and truncating"""
    heads = set(itertools.product((0, 1, 2, 3), (1, 2, 3)))
    want = {h + o for h in heads for o in OUT_CLASSES} - {(0, 1) + DIGEST_OUT, (2, 1) + DIGEST_OUT}
    assert len(want) == 12 * 9 - 2
    for line_fetch in (True, False):
        seen = _sponge_classes(S.N_ONE_LANE, 0, line_fetch)
        assert seen["k_sponge"] == want and seen["k_sponge_trunc"] == want
        assert set(seen) == ({"k_sponge", "k_sponge_trunc", "k_sponge_lines", "k_sponge_lines_trunc"} if line_fetch else {"k_sponge", "k_sponge_trunc"})
    # the lane-group kernels take every shape in every layout (their lanes fetch scalar by scalar: the same classes)
    seen = _sponge_classes(S.N_LANE_GROUPS, 16384, True)
    assert set(seen) == {"k_sponge_coop", "k_sponge_coop_trunc"} and seen["k_sponge_coop"] == want and seen["k_sponge_coop_trunc"] == want


def test_the_sponge_lane_model_restates_the_kernel():
    """hand-worked lanes of sponge_body<true> (kernels.hip): 42 scalars as allocated — lane 0 starts on a line and ends two scalars into
    one, fetched at trip 10; lane 1 starts there and ends on a line; 4 scalars at +64 B: every lane parks at trip 0"""
    assert S.sponge_lane(42, 5, 0, 0, True) == {"sh": 0, "tail_half": True, "parked": 10, "absorb_blocks": 11, "squeeze_blocks": 2}
    assert S.sponge_lane(42, 5, 0, 1, True) == {"sh": 2, "tail_half": False, "parked": None, "absorb_blocks": 11, "squeeze_blocks": 2}
    assert S.sponge_lane(4, 7, 64, 5, True) == {"sh": 2, "tail_half": True, "parked": 0, "absorb_blocks": 1, "squeeze_blocks": 2}
    assert S.sponge_lane(8, 9, 64, 3, True) == {"sh": 2, "tail_half": True, "parked": 1, "absorb_blocks": 2, "squeeze_blocks": 3}
    assert S.sponge_lane(2, 2, 0, 1, True)["sh"] == 2 and S.sponge_lane(2, 2, 0, 0, True)["parked"] == 0
    assert S.sponge_lane(7, 2, 32, 1, False) == {"sh": 0, "tail_half": False, "parked": None, "absorb_blocks": 2, "squeeze_blocks": 1}
    # launch_sponge: lane groups up to 8,192 messages; whole lines for even lengths on a 64-byte boundary, unless switched off
    assert S.sponge_kernel(70, 42, 5, 0, False) == "k_sponge_coop" and S.sponge_kernel(70, 42, 5, 0, True) == "k_sponge_coop_trunc"
    assert S.sponge_kernel(8193, 42, 5, 0, False) == "k_sponge_lines" and S.sponge_kernel(8193, 42, 5, 64, True) == "k_sponge_lines_trunc"
    assert S.sponge_kernel(8193, 42, 5, 32, False) == "k_sponge" and S.sponge_kernel(8193, 41, 5, 0, False) == "k_sponge"
    assert S.sponge_kernel(323, 42, 5, 0, False, coop_max=0) == "k_sponge_lines"
    assert S.sponge_kernel(323, 42, 5, 0, True, coop_max=0, line_fetch=False) == "k_sponge_trunc"


# ---------------------------------------------------------------------------------------------- the cipher
def test_cipher_classes_are_all_reached():
    """every (variant, len mod 4) with 1, 2 and 3-or-more permutations inside the message, where the state machine has them: STREAM
    squeezes ceil(len / 4) times and absorbs from position 0, 2 ceil(len / 4) - 1 permutations — never two; DUPLEX permutes once per
    chunk.  The MAC squeeze follows an absorb call, which leaves the squeeze position at 4: it ALWAYS permutes first (the machine
    does not allow the other case, and the equality below says so)."""
    want = {(STREAM, r, c, True) for r in (0, 1, 2, 3) for c in (1, 3)} | {(DUPLEX, r, c, True) for r in (0, 1, 2, 3) for c in (1, 2, 3)}
    assert len(want) == 20
    assert {S.crypt_class(v, ln) for v, ln in S.CRYPT_CASES} == want
    # and no length at all gives another class
    assert {S.crypt_class(v, ln) for v in (STREAM, DUPLEX) for ln in range(1, 200)} == want
    # the secret scalars and the nonce take absorb positions 0 .. 2; the first mask's squeeze permutes and resets both positions, so the
    # masks are squeezed, and the message absorbed, from position 0
    for v, ln in S.CRYPT_CASES:
        walk = S.crypt_walk(v, ln)
        assert walk[:3] == [(0, 0, False), (0, 1, False), (1, 2, False)] and walk[3] == (2, 0, True)
        assert len(walk) == 3 + 2 * ln + 1 and walk[-1] == (4, 0, True)
        assert [p for k, p, _ in walk if k == 2] == [e % 4 for e in range(ln)]  # the lane-group build: lane 1 + position
    assert S.crypt_kernel(70) == "k_crypt_coop" and S.crypt_kernel(323, 0) == "k_crypt" and S.crypt_kernel(8193) == "k_crypt"


def test_cipher_program_is_the_io_pattern_of_the_bigint_machine():
    import pymodel as T
    for v, ln in S.CRYPT_CASES:
        assert [("A" if k in (0, 1, 3) else "S", c) for k, c in S.crypt_program(v, ln)] == T._io_pattern(v, ln)


# ---------------------------------------------------------------------------------------------- the paths
def test_path_classes_and_kernels_are_all_reached():
    """depth 0 and 1, every residue mod 4 below 4, from 4 to 7 and above 8 — both neighbours of 4, 8 and 12 among them — for both
    arities; the whole-line kernel with one to four position words and with a second fetch of them; every layout on the kernel the
    launcher picks for it"""
    want = set(itertools.product((4, 2), (0, 1, 2, 3), (0, 1, 2)))
    assert {(a,) + S.path_class(d) for a, d in S.PATH_CASES} == want
    assert S.path_class(0) == (0, 0) and S.path_class(1) == (1, 0)
    assert [d for d in S.PATH_DEPTHS if S.path_class(d) == (0, 0)] == [0] and [d for d in S.PATH_DEPTHS if S.path_class(d) == (1, 0)] == [1]
    assert {m + s for m in (4, 8, 12) for s in (-1, 0, 1)} <= set(S.PATH_DEPTHS)

    def reached(n, coop_max, line_fetch):
        seen = {}
        for (a, d), lay in itertools.product(S.PATH_CASES, S.PATH_LAYOUTS):
            seen.setdefault(S.path_kernel(a, n, d, lay, coop_max, line_fetch), set()).add((lay, d))
        return seen

    every = {(lay, d) for lay in S.PATH_LAYOUTS for d in S.PATH_DEPTHS}
    lines = {("aligned", d) for d in (4, 8, 12, 16, 20)}
    assert reached(S.N_LANE_GROUPS, 16384, True) == {"k_merkle4_path_coop": every, "k_merkle2_path": every}
    assert reached(S.N_ONE_LANE, 0, True) == {"k_merkle4_path_lines": lines, "k_merkle4_path": every - lines, "k_merkle2_path": every}
    assert reached(S.N_ONE_LANE, 0, False) == {"k_merkle4_path": every, "k_merkle2_path": every}
    assert {S.path_lines_class(d) for _, d in lines} == {(1, False), (2, False), (3, False), (4, False), (4, True)}


def test_predicted_kernels_per_environment():
    """what the GPU file's three environments must find in their kernel traces"""
    sponge_one = {"k_sponge", "k_sponge_trunc", "k_sponge_ragged", "k_sponge_ragged_trunc"}
    assert S.predicted_kernels("sponge", 70, 16384, True) == {"k_sponge_coop", "k_sponge_coop_trunc", "k_sponge_ragged_coop", "k_sponge_ragged_coop_trunc"}
    assert S.predicted_kernels("sponge", 323, 0, True) == sponge_one | {"k_sponge_lines", "k_sponge_lines_trunc"}
    assert S.predicted_kernels("sponge", 323, 0, False) == sponge_one
    assert S.predicted_kernels("crypt", 70, 16384, True) == {"k_crypt_coop"} and S.predicted_kernels("crypt", 323, 0, True) == {"k_crypt"}
    assert S.predicted_kernels("paths", 70, 16384, True) == {"k_merkle4_path_coop", "k_merkle2_path", "k_path_ragged"}
    assert S.predicted_kernels("paths", 323, 0, True) == {"k_merkle4_path", "k_merkle4_path_lines", "k_merkle2_path", "k_path_ragged"}
    assert S.predicted_kernels("paths", 323, 0, False) == {"k_merkle4_path", "k_merkle2_path", "k_path_ragged"}
    assert S.expected_rows("sponge", 323) == 323 * (180 * 6 + 36) and S.expected_rows("crypt", 70) == 70 * 126
    assert S.expected_rows("paths", 323) == 323 * 128


def test_the_tampered_copy_hits_every_element():
    c = np.zeros((S.N_LANE_GROUPS, 44, 4), dtype=np.uint64)
    rows, elems = np.nonzero(S.tampered(c).any(axis=2))
    assert np.array_equal(rows, np.arange(S.N_LANE_GROUPS)) and set(elems.tolist()) == set(range(44)) and np.array_equal(elems, rows % 44)
    assert int(S.tampered(c).sum()) == 4 * S.N_LANE_GROUPS  # one bit each


# ---------------------------------------------------------------------------------------------- the oracle at these shapes
@pytest.fixture(scope="module")
def perm():
    C, M = pymodel.load_constants()
    return lambda s: pymodel.perm_reference(s, C, M)


def test_oracle_sponge_matches_the_bigint_sponge_at_every_shape(oracle_mod, perm):
    """every shape of the sweep (none thinned out), one message each: oracle.hash_batch against pymodel.sponge"""
    f = oracle_mod.int_from_mont
    for in_len, out_len in S.SPONGE_SHAPES:
        tag = oracle_mod.tag(3, [in_len], out_len)
        msg = oracle_mod.fill_random(1000 * in_len + out_len, in_len)
        got = [f(v) for v in oracle_mod.hash_batch(tag, msg, in_len, out_len)[0]]
        assert got == pymodel.sponge(f(tag), [f(v) for v in msg], out_len, perm), (in_len, out_len)


def test_oracle_encryption_matches_the_bigint_machine_at_every_case(oracle_mod, perm):
    """every (variant, len) of the sweep: the oracle's encrypt against the big-integer state machine of tests/pymodel.py, whose
    count of permutations is the dispatch model's"""
    f = oracle_mod.int_from_mont
    for variant, ln in S.CRYPT_CASES:
        tag = oracle_mod.encryption_tag(ln, variant)
        msg = oracle_mod.fill_random(7000 + 2 * ln + variant, ln)
        secret, nonce = oracle_mod.fill_random(8000 + ln, 2), oracle_mod.fill_random(9000 + ln, 1)[0]
        calls = []

        def counted(s):
            calls.append(1)
            return perm(s)

        want = S.bigint_encrypt(variant, f(tag), [f(v) for v in msg], [f(secret[0]), f(secret[1])], f(nonce), counted)
        got = [f(v) for v in oracle_mod.encrypt_batch(tag, msg[None], secret[None], nonce[None], variant)[0]]
        assert got == want, (variant, ln)
        assert len(calls) == sum(1 for _, _, permutes in S.crypt_walk(variant, ln) if permutes), (variant, ln)
