"""The argument refusals of every `_device` entry point, as a table that needs no GPU (tests/cpp/api_refusals.cpp): one context that
never saw a device reaches every check the C ABI makes before hipSetDevice.  The program's lines are compared with
tests/golden/api_refusals.txt — refusals and early P252_OK byte for byte; rows that got past validation (the control row of every
entry point, and varied rows the library accepts) by return code and by the part of the message that is the library's, up to the
first ": " (the rest is the HIP runtime's and differs between machines)."""
import os
import re

import pytest

from helpers.percall import ERR_HIP, assert_rows_equal_golden, refusal_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the one entry point that takes a communicator, which only RCCL ranks can make: no argument set of it gets past validation here
NO_CONTROL = {"p252_merkle4_tree_sharded_device"}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("api_refusals", tmp_path_factory.mktemp("api_refusals"))


def test_every_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "api_refusals")


def test_every_entry_point_has_a_control_row_that_reaches_the_device(table):
    control = {r[0]: r for r in table if r[1] == "control"}
    assert set(control) == {r[0] for r in table} - NO_CONTROL
    for sym, (_, _, rc, msg) in control.items():  # without this the one-at-a-time rows prove nothing
        assert rc == ERR_HIP and msg.startswith("hipSetDevice"), (sym, rc, msg)
        # (p252_merkle4_tree_multi_device binds each context's device itself and reports plain "hipSetDevice")
        assert msg == "hipSetDevice(ctx->device)" or sym == "p252_merkle4_tree_multi_device", (sym, msg)


def test_every_other_row_is_a_refusal_an_empty_call_or_accepted(table):
    for sym, case, rc, msg in table:
        if case == "control":
            continue
        assert rc in (0, -1, -2, -3, ERR_HIP), (sym, case, rc)
        if rc == 0:
            assert msg == "", (sym, case, msg)  # nothing was tried
        if rc == ERR_HIP:  # accepted: past validation, stopped where the control row stops
            assert msg.startswith("hipSetDevice"), (sym, case, msg)


def test_verify_batch_refuses_what_path_batch_refuses(table):
    """the re-hash's own checks run before p252_merkle{4,2}_verify_batch_device binds the device or takes scratch"""
    by = {(r[0], r[1]): r[2:] for r in table}
    cases = [c for (s, c) in by if s == "p252_merkle4_path_batch_device" and c not in ("control", "ctx=NULL") and not c.startswith(("d_roots", "n="))]
    assert len(cases) >= 15
    for arity in "42":
        for case in cases:
            assert by[("p252_merkle%s_verify_batch_device" % arity, case)] == by[("p252_merkle%s_path_batch_device" % arity, case)], (arity, case)


def test_every_device_symbol_of_the_header_is_in_the_table(table):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))
    assert len(declared) >= 40
    assert declared == {r[0] for r in table}


def test_depths_of_both_arities_and_their_wrap_at_the_top_of_size_t():
    """p252_merkle{4,2}_depth share one loop; `c + arity - 1` wraps at SIZE_MAX, which is ABI: the depth of SIZE_MAX leaves stays 1"""
    from poseidon252_amd import _lib
    L = _lib.lib()
    for arity, fn in ((4, L.p252_merkle4_depth), (2, L.p252_merkle2_depth)):
        for n, want in ((0, 0), (1, 0), (2, 1), (arity, 1), (arity + 1, 2), (arity ** 5, 5), (arity ** 5 + 1, 6), (2 ** 32, 64 // arity)):
            assert fn(n) == want, (arity, n)
        assert fn(2 ** 64 - 1) == 1, arity
