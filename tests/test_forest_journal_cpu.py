"""The journaled leaf update of a ragged forest and its swap (p252_merkle{4,2}_forest_ragged_journal_bound, _update_journaled_device_into,
_journal_swap_device_into; csrc/forest_journal.hip) — what can be checked without a GPU: the six entry points are declared, exported and
mirrored in the Rust FFI under ABI 9; the host bound is the documented formula, covers the numpy model of the journal and is met
where no two updates share an ancestor; forest_journal.hip compiles for gfx950 to its three bookkeeping kernels within their
resource targets and brings no digest of its own; the Python mirror refuses a CPU tensor before the library is reached and adds no
arity= parameter; the argument refusals of the two device entry points equal a recorded table; the C++ mirror test compiles."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")

import forestjournal as FJ  # noqa: E402
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401
from helpers.forest import _mix, dirty_count  # noqa: E402
from helpers.kernel_resources import kernel_resources  # noqa: E402
from helpers.percall import (ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols,  # noqa: E402
                             refusal_table)
from testsupport import treeshape as TS  # noqa: E402

ARGS = {"p252_merkle%d_forest_ragged_%s" % (a, stem): n for a in (4, 2)
        for stem, n in (("journal_bound", 4), ("update_journaled_device_into", 20), ("journal_swap_device_into", 14))}
STEMS = ("journal_bound", "update_journaled_device", "journal_swap_device")


def test_six_symbols_declared_exported_and_in_sys_rs():
    assert len(ARGS) == 6
    raw, header = check_abi_symbols(ARGS)
    # the update's arguments first, in its order, then the journal's four, then the stream
    plain = re.search(r"\bint p252_merkle4_forest_ragged_update_device\s*\((.*?)\);", header, flags=re.S).group(1)
    journaled = re.search(r"\bint p252_merkle4_forest_ragged_update_journaled_device_into\s*\((.*?)\);", header, flags=re.S).group(1)
    norm = lambda s: [re.sub(r"\s+", " ", p.strip()) for p in s.split(",")]  # noqa: E731
    assert norm(journaled)[:15] == norm(plain)[:15] and norm(journaled)[-1] == norm(plain)[-1] == "void* hip_stream"
    assert norm(journaled)[15:19] == ["void* d_journal_ids", "void* d_journal_values", "size_t journal_cap", "void* d_journal_len"]
    # the header says what voids a journal, and the version history names the addition
    assert "ONLY MEANINGFUL FOR THE FOREST SHAPE" in raw and "void every older journal" in raw
    assert re.search(r"_journal_swap_device_into \(additive, same\s+\*\s+version", raw)


def _bound(arity):
    from poseidon252_amd import _lib
    fn = getattr(_lib.lib(), "p252_merkle%d_forest_ragged_journal_bound" % arity)
    return lambda *a: int(fn(*a))


@pytest.mark.parametrize("arity", [4, 2])
def test_bound_is_the_formula_and_covers_the_model(arity):
    bound = _bound(arity)
    rng = np.random.default_rng(100 + arity)
    # the formula, zero sizes and saturation included
    for n_leaves, n_trees, max_leaves, k in [(1, 1, 1, 1), (4 ** 12, 1, 4 ** 12, 1), (4 ** 12, 1, 4 ** 12, 1 << 20), (2 ** 24, 1, 2 ** 24, 77),
                                             (100, 7, 16, 5), (100, 7, 1000, 5), (1 << 40, 20000, 1 << 30, 1 << 33), (3, 1, 2, 9)]:
        assert bound(n_leaves, n_trees, max_leaves, k) == FJ.journal_bound(n_leaves, n_trees, max_leaves, k, arity)
    for zero in range(4):
        a = [10, 2, 5, 3]
        a[zero] = 0
        assert bound(*a) == 0
    top = FJ.SIZE_MAX
    assert bound(top, top, top, top) == top and bound(top // 2, 5, top, top) == top
    assert bound(top, 1, 1, top) == top  # (depth 0: the leaves alone)
    assert bound(top // 64, 1, top, 1) == FJ.journal_bound(top // 64, 1, top, 1, arity) < 200
    # >= the model's count, which is the distinct valid pairs plus the dirty nodes
    sizes = _mix(arity) * 2
    n_leaves, n_trees, max_leaves = sum(sizes) + 8, len(sizes), max(sizes)
    for case in range(300):
        k = int(rng.integers(1, 700))
        tid = rng.integers(0, n_trees + 1, k)  # (ids past the forest among them)
        lid = rng.integers(0, [3, 70, max_leaves + 2][case % 3], k)  # (repeats, and ids past the small trees)
        entries = FJ.journal_entries(sizes, arity, tid, lid)
        valid = {(t, i) for t, i in zip(tid.tolist(), lid.tolist()) if t < n_trees and i < sizes[t]}
        assert len(entries) == len(valid) + dirty_count(sizes, tid, lid, arity), case
        assert sum(1 for e in entries if e[1] == 0) == len(valid)
        assert len(entries) <= bound(n_leaves, n_trees, max_leaves, k), case


@pytest.mark.parametrize("arity", [4, 2])
def test_bound_is_met_when_no_two_updates_share_an_ancestor(arity):
    bound = _bound(arity)
    for d, T in ((0, 5), (1, 3), (3, 17), (5, 2)):
        n = arity ** d
        sizes = [n] * T
        tid, lid = np.arange(T), (np.arange(T) * 7) % n  # one leaf per tree
        entries = FJ.journal_entries(sizes, arity, tid, lid)
        assert len(entries) == T * (d + 1) == bound(T * n, T, n, T), (d, T)
    # one more update must share every ancestor above some level: the bound is then strictly above the count
    assert len(FJ.journal_entries([arity ** 3], arity, [0, 0], [0, 1])) == 2 + 3 < bound(arity ** 3, 1, arity ** 3, 2)


def test_host_swap_model_is_an_involution():
    arity, sizes = 4, [1, 5, 17, 0, 64]
    off = np.concatenate([[2], 2 + np.cumsum(sizes)]).astype(np.uint64)
    rng = np.random.default_rng(3)
    leaves = rng.integers(0, 1 << 62, (int(off[-1]) + 1, 4)).astype(np.uint64)
    levels = [rng.integers(0, 1 << 62, (TS.levels_len(n, arity), 4)).astype(np.uint64) for n in sizes]
    want = sorted(FJ.journal_entries(sizes, arity, [0, 2, 2, 4, 4, 9, 3], [0, 16, 3, 63, 0, 0, 0]), key=lambda e: (e[1], e[0], e[2]))
    ids = np.array([[t, lv + 1, i & 0xFFFFFFFF, i >> 32] for t, lv, i in want] + [[0, 0, 0, 0], [1, 4, 0, 0], [2, 1, 17, 0], [3, 1, 0, 0]], np.uint32)
    values = rng.integers(0, 1 << 62, (len(ids), 4)).astype(np.uint64)
    l0, lv0, v0 = leaves.copy(), [x.copy() for x in levels], values.copy()
    roots = np.zeros((len(sizes), 4), np.uint64)
    assert FJ.swap_host(leaves, off, sizes, levels, ids, values, len(ids), arity, roots, reduce=lambda x: x) == 4
    assert not np.array_equal(leaves, l0) and np.array_equal(values[len(want):], v0[len(want):])
    assert np.array_equal(roots[0], v0[0]) and np.array_equal(roots[2], levels[2][-1]) and not np.array_equal(levels[2][-1], lv0[2][-1])
    assert not roots[1].any() and not roots[3].any()
    assert FJ.swap_host(leaves, off, sizes, levels, ids, values, len(ids), arity) == 4
    assert np.array_equal(leaves, l0) and np.array_equal(values, v0) and all(np.array_equal(a, b) for a, b in zip(levels, lv0))


@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_journal.hip", os.path.join(CSRC, "_gen", "forest_journal_test.s"))


def test_three_bookkeeping_kernels_within_their_resource_targets(compiled):
    res, isa = compiled
    for kernel in ("k_fj_leaves", "k_fj_claim", "k_fj_swap"):
        assert sum(1 for n in res if kernel in n) == 1, (kernel, sorted(res))
    assert len(res) == 3, sorted(res)  # and no digest kernel of its own
    for name, v in res.items():
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    assert "scratch_" not in isa


def test_own_translation_unit_and_nothing_is_copied():
    from poseidon252_amd import build as b
    assert "forest_journal.hip" in b.SOURCES and "forest_journal.h" in b.HEADERS
    src = open(os.path.join(CSRC, "forest_journal.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "forest_node.hpp"' in src and '#include "forest_update.h"' in src
    # the digests are the update's — reached through its level loop (forest_update.h), which is handed k_fj_claim's launch — and the address
    # arithmetic forest_node.hpp's: used here, defined there
    levels = re.search(r"\blaunch_forest_update_levels\s*\([^;{]*\)\s*\{.*?\n\}", open(os.path.join(CSRC, "forest_update.h")).read(), flags=re.S)
    assert levels and "launch_forest_digest_list(" in levels.group(0) and "enqueue_claim(" in levels.group(0)
    assert "launch_forest_update_levels(" in code and not re.search(r"hipError_t\s+launch_forest_update_levels\b", code)
    assert "hades_permute" not in code and "node_digest_coop" not in code
    for fn in ("level_start", "ceil_shift", "u64_of", "forest_tree_leaves", "level_nodes"):
        assert re.search(r"\b%s\(" % fn, code), fn
        assert not re.search(r"\b%s\s*\([^;{]*\)\s*\{" % fn, code), fn
    assert not re.search(r"\bk_f[ur]_\w+\s*[(<]", code)  # no kernel of the update's or the build's is launched or copied
    assert "launch_forest_ragged_index" in open(os.path.join(CSRC, "api_forest.cpp")).read()
    assert "asm" not in src  # plain C++ and vector stores only
    for other in ("kernels.hip", "kernels.h", "forest_update.hip", "forest_update.h"):
        assert "forest_journal" not in open(os.path.join(CSRC, other)).read(), other


def _cases(c):
    """(the C entry point, the call, its arguments) for the four methods that hand device pointers to the library.  d_leaves is 16
    scalars long, which sets the bound of d_levels; the journal holds 8 entries."""
    tag = np.zeros(4, dtype=np.uint64)
    i32 = torch.int32
    forest = dict(d_leaves=dev(), d_offsets=dev(), d_levels=dev(n=256))
    journal = dict(d_journal_ids=dev(i32), d_journal_values=dev(), d_journal_len=dev())
    out = []
    for arity in (4, 2):
        upd = getattr(c, "merkle%d_forest_ragged_update_journaled_device" % arity)
        swap = getattr(c, "merkle%d_forest_ragged_journal_swap_device" % arity)
        out.append(("p252_merkle%d_forest_ragged_update_journaled_device_into" % arity, lambda a, upd=upd: upd(
            tag, a["d_leaves"], a["d_offsets"], 2, 4, a["d_levels"], a["d_tree_ids"], a["d_leaf_ids"], a["d_new_leaves"], 2, a["d_journal_ids"],
            a["d_journal_values"], 8, a["d_journal_len"], a["d_roots"], a["d_n_bad"], a["d_n_hashed"]),
            dict(forest, d_tree_ids=dev(i32), d_leaf_ids=dev(), d_new_leaves=dev(), d_roots=dev(), d_n_bad=dev(i32), d_n_hashed=dev(), **journal)))
        out.append(("p252_merkle%d_forest_ragged_journal_swap_device_into" % arity, lambda a, swap=swap: swap(
            a["d_leaves"], a["d_offsets"], 2, 4, a["d_levels"], a["d_journal_ids"], a["d_journal_values"], 8, a["d_journal_len"], a["d_roots"],
            a["d_n_bad"]), dict(forest, d_roots=dev(), d_n_bad=dev(i32), **journal)))
    return out


def test_every_new_device_pointer_refuses_a_cpu_tensor(recorder):
    n_refused = 0
    for symbol, call, args in _cases(_no_device_context()):
        call(args)  # the control: with every tensor "on the device" the call reaches the library, once
        assert recorder.calls == [symbol], (symbol, recorder.calls)
        del recorder.calls[:]
        for where, bad in with_cpu_tensor(args):
            with pytest.raises(ValueError, match="is on cpu") as e:
                call(bad)
            assert where + " is on cpu" in str(e.value), (symbol, where, str(e.value))
            assert recorder.calls == [], (symbol, where, recorder.calls)
            n_refused += 1
    assert n_refused == 2 * (12 + 8)


def test_the_journal_is_sized_by_its_capacity(recorder):
    """journal_cap x 16 and journal_cap x 32 bytes: a journal one entry short is refused before the library is reached"""
    c = _no_device_context()
    for symbol, call, args in _cases(c):
        for name, short, match in (("d_journal_ids", dev(torch.int32, n=8 * 4 - 1), "holds 124 bytes, the call touches 128"),
                                   ("d_journal_values", dev(n=8 * 4 - 1), "holds 248 bytes, the call touches 256"),
                                   ("d_journal_ids", dev(n=16), "needs 4-byte elements"),
                                   ("d_journal_len", dev(torch.int32), "needs 8-byte elements")):
            with pytest.raises(ValueError, match=match):
                call(dict(args, **{name: short}))
        with pytest.raises(ValueError, match="d_journal_len must be a torch tensor"):  # required, unlike the counters
            call(dict(args, d_journal_len=None))
        call(dict(args, d_roots=None, d_n_bad=None, **({"d_n_hashed": None} if "d_n_hashed" in args else {})))
        assert recorder.calls == [symbol]
        del recorder.calls[:]


# ---- the refusals of the two device entry points, as a table that needs no GPU (tests/cpp/journal_refusals.cpp) ----
DEVICE_SYMBOLS = [n for n in ARGS if n.endswith("_device_into")]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("journal_refusals", tmp_path_factory.mktemp("journal_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "journal_refusals")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    assert sorted({r[0] for r in table}) == sorted(DEVICE_SYMBOLS) and len(DEVICE_SYMBOLS) == 4
    for sym in DEVICE_SYMBOLS:
        by = {r[1]: r[2:] for r in table if r[0] == sym}
        arity, update = int(sym[len("p252_merkle")]), "update_journaled" in sym
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3
        for rc, msg in by.values():
            assert rc in (0, -3, ERR_HIP) and (rc != 0 or msg == "") and (rc != ERR_HIP or msg == "hipSetDevice(ctx->device)")
        required = ["d_leaves", "d_offsets", "d_levels", "d_journal_ids", "d_journal_values", "d_journal_len"]
        required += ["tag", "d_tree_ids", "d_leaf_ids", "d_new_leaves"] if update else []
        for buf in required:
            assert refused(buf + "=NULL", "NULL buffer"), (sym, buf)
        for buf in ["d_roots", "d_n_bad"] + (["d_n_hashed"] if update else []):
            assert accepted(buf + "=NULL"), (sym, buf)
        for buf in ("d_leaves+8", "d_levels+8", "d_roots+8", "d_journal_ids+8", "d_journal_values+8"):
            assert refused(buf, "16-byte aligned"), (sym, buf)
        assert refused("d_journal_len+4", "8-byte aligned") and refused("d_offsets+4", "8-byte aligned") and refused("d_n_bad+2", "4-byte aligned")
        for case in ("n_leaves=0", "n_trees=0", "max_leaves=0"):
            assert refused(case, "must be > 0"), (sym, case)
        for case in ("n_leaves=SIZE_MAX/64+1", "n_trees=SIZE_MAX/8/66+1", "journal_cap=0x400000000000000"):
            assert refused(case, "size overflow"), (sym, case)
        assert accepted("n_leaves=SIZE_MAX/64") and accepted("max_leaves=1,d_levels=NULL")
        if update:
            # the journal's capacity at both sides of the call's bound (n_leaves 12, n_trees 3, max_leaves 5, k 7), and of a forest without levels
            bound = FJ.journal_bound(12, 3, 5, 7, arity)
            assert refused("journal_cap=" + hex(bound - 1), "journal_cap %d is below the call's bound of %d" % (bound - 1, bound))
            assert accepted("journal_cap=" + hex(bound)) and refused("journal_cap=0", "below the call's bound")
            assert accepted("max_leaves=1,journal_cap=7") and refused("max_leaves=1,journal_cap=6", "bound of 7")
            assert refused("k=SIZE_MAX/128+1", "size overflow") and refused("k=SIZE_MAX/128", "below the call's bound")
            # k == 0 sets the length and nothing else: the journal's buffers may be NULL, the length may not
            assert accepted("k=0") and accepted("k=0,journal_cap=0,d_journal_ids=d_journal_values=NULL") and refused("k=0,d_journal_len=NULL", "NULL buffer")
        else:
            assert by["journal_cap=0"] == (0, "") and by["journal_cap=0,every buffer NULL"] == (0, "")  # nothing enqueued
            assert accepted("journal_cap=0x3ffffffffffffff") and accepted("n_leaves=1,d_levels=NULL")


def test_public_methods_are_per_arity_without_an_arity_parameter():
    from poseidon252_amd import Context
    for arity in (4, 2):
        for stem in STEMS:
            m = getattr(Context, "merkle%d_forest_ragged_%s" % (arity, stem))
            assert "arity" not in inspect.signature(m).parameters, m
    for stem in STEMS:  # one method each behind the two names, which takes the arity last
        last = list(inspect.signature(getattr(Context, "merkle_forest_ragged_" + stem)).parameters.values())[-1]
        assert last.name == "arity" and last.default == 4, stem
    import poseidon252_amd as P
    from poseidon252_amd import merkle as M
    assert list(inspect.signature(M.forest_ragged_update_journaled).parameters) == [
        "ctx", "tag", "d_leaves", "d_offsets", "n_trees", "max_leaves", "d_levels", "tree_ids", "leaf_ids", "new_leaves", "d_roots", "arity"]
    assert list(inspect.signature(M.forest_ragged_journal_swap).parameters) == [
        "ctx", "d_leaves", "d_offsets", "n_trees", "max_leaves", "d_levels", "journal", "d_roots", "arity"]
    assert "forest_ragged_update_journaled" in P.__all__ and "forest_ragged_journal_swap" in P.__all__


def test_bound_method_reaches_the_host_function():
    c = _no_device_context()
    assert c.merkle4_forest_ragged_journal_bound(4 ** 6, 1, 4 ** 6, 3) == FJ.journal_bound(4 ** 6, 1, 4 ** 6, 3, 4) == 3 * 6 + 2  # (the top level's bound is n / a^6 + n_trees = 2)
    assert c.merkle2_forest_ragged_journal_bound(2 ** 6, 1, 2 ** 6, 3) == FJ.journal_bound(2 ** 6, 1, 2 ** 6, 3, 2) == 3 * 6 + 2


def test_cpp_mirror_test_compiles(tmp_path):
    build_cpp_mirror("test_forest_journal_api", tmp_path, oracle=False)


def test_bench_tool_parses():
    bench_tool_parses("forest_journal_bench")
