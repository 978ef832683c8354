"""The argument refusals of the host-buffer entry points (csrc/host_io.cpp) and of p252_scratch_residue / p252_tables_export /
p252_tables_import, as a table that needs no GPU (tests/cpp/host_refusal_table.cpp), compared with tests/golden/host_refusals.txt as
tests/test_api_refusals_cpu.py compares the `_device` calls' table: refusals and early P252_OK byte for byte, rows that got past
validation by return code and by the library's part of the message."""
import pytest

from helpers.percall import ERR_HIP, assert_rows_equal_golden, refusal_table

# its control row is a refusal as well: the one table p252_tables_import accepts comes out of a device
NO_CONTROL = {"p252_tables_import"}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("host_refusal_table", tmp_path_factory.mktemp("host_refusals"))


def test_every_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "host_refusals")


def test_every_entry_point_has_a_control_row_that_reaches_the_device(table):
    control = {r[0]: r for r in table if r[1] == "control"}
    assert set(control) == {r[0] for r in table} and len(control) == 18
    for sym, (_, _, rc, msg) in control.items():  # without this the one-at-a-time rows prove nothing
        if sym not in NO_CONTROL:
            assert rc == ERR_HIP and msg == "hipSetDevice(ctx->device)", (sym, rc, msg)
    for sym, case, rc, msg in table:
        assert rc in (0, -2, -3, ERR_HIP) and (rc != 0 or msg == ""), (sym, case, rc, msg)
