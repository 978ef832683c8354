"""Trees of built forests gathered into a new forest (p252_merkle{4,2}_forest_ragged_select_device_into; the select of
csrc/forest_ragged.hip) — what can be checked without a GPU: the two entry points are declared, exported and mirrored in the Rust FFI
under ABI 9, under a name the refusal table of the `_device(` symbols does not catch; the host refusals as a table of their own; the
select's kernels compile for gfx950 within
their resource targets and none of them hashes; the Python methods validate every buffer before the library is reached; the model
the GPU tests compare the call with; the C++ mirror compiles; the bench tool parses."""
import os
import re

import numpy as np
import pytest
import torch

import forestselect as FS
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: F401
from helpers.kernel_resources import kernel_resources
from helpers.percall import ERR_HIP, assert_rows_equal_golden, bench_tool_parses, build_cpp_mirror, check_abi_symbols, refusal_table
from testsupport import treeshape as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")
SYMBOLS = ("p252_merkle4_forest_ragged_select_device_into", "p252_merkle2_forest_ragged_select_device_into")
N_ARGS = 25


# ---- the symbols ----
def test_two_symbols_declared_exported_and_in_sys_rs():
    _, header = check_abi_symbols(dict.fromkeys(SYMBOLS, N_ARGS))
    # no new name that the refusal table of the `_device(` symbols would have to hold: that table stays as it is
    declared = set(re.findall(r"\b(p252_[a-z0-9_]+_device)\s*\(", header))
    table = {line.split("\t")[0] for line in open(os.path.join(ROOT, "tests", "golden", "api_refusals.txt")).read().splitlines()}
    assert declared == table and not any("select" in s for s in declared)


# ---- the host refusals (the library's own: the table of the `_device(` symbols does not see a `_device_into` name) ----
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return refusal_table("select_refusals", tmp_path_factory.mktemp("select_refusals"))


def test_every_refusal_row_equals_the_recorded_one(table):
    assert_rows_equal_golden(table, "select_refusals")


SELECT_IN = ("d_leaves_a", "d_offsets_a", "d_levels_a", "d_roots_a", "d_leaves_b", "d_offsets_b", "d_levels_b", "d_roots_b", "d_pick")
SELECT_OUT = ("d_leaves_new", "d_offsets_new", "d_levels_new", "d_roots_new", "d_n_bad")


def test_refusal_table_has_a_control_row_and_every_host_refusal(table):
    for arity in (4, 2):
        by = {r[1]: r[2:] for r in table if r[0] == "p252_merkle%d_forest_ragged_select_device_into" % arity}
        assert by["control"] == (ERR_HIP, "hipSetDevice(ctx->device)")  # past validation: without this the other rows prove nothing
        refused = lambda case, word: by[case][0] == -3 and word in by[case][1]  # noqa: E731
        accepted = lambda case: by[case] == by["control"]  # noqa: E731
        assert by["ctx=NULL"][0] == -3 and refused("n_trees_a=0", "n_trees_a must be > 0")
        assert by["n_pick=0"] == (0, "") and by["n_pick=0,n_leaves_a=0,buffers=NULL"] == (0, "")
        # B absent: accepted whatever its pointers and sizes say
        for case in ("n_trees_b=0,B=NULL", "n_trees_b=0", "n_trees_b=0,B misaligned", "n_trees_b=0,B on the outputs",
                     "n_trees_b=0,n_leaves_b=0,max_leaves_b=0", "n_trees_b=0,max_leaves_b=17", "n_trees_b=0,n_pick*min(max_leaves_b,n_leaves_b)>SIZE_MAX/2"):
            assert accepted(case) or (case.endswith("SIZE_MAX/2") and refused(case, "levels_cap must be >=")), (case, by[case])
        assert refused("n_leaves_b=0", "n_leaves_b and max_leaves_b must be > 0") and refused("max_leaves_b=0", "n_leaves_b and max_leaves_b must be > 0")
        assert refused("n_leaves_a=0", "n_leaves_a and max_leaves_a must be > 0") and refused("max_leaves_a=0", "n_leaves_a and max_leaves_a must be > 0")
        assert refused("leaves_cap=0", "leaves_cap must be > 0")
        # the levels' cap: one below the bound and at it, under the larger of the two max_leaves
        for case in ("levels_cap=need-1", "levels_cap=0", "max_leaves_a=17", "max_leaves_a=17,levels_cap=need(17)-1", "max_leaves_b=17,levels_cap=need(17)-1"):
            assert refused(case, "levels_cap must be >= leaves_cap / (arity - 1) + n_pick * depth(max_leaves)"), case
        for case in ("levels_cap=need", "levels_cap=need+1", "max_leaves_a=17,levels_cap=need(17)", "max_leaves_b=17,levels_cap=need(17)"):
            assert accepted(case), case
        assert accepted("max_leaves_a=1,d_levels_a=NULL") and accepted("max_leaves_b=1,d_levels_b=NULL") and accepted("max_leaves_a=max_leaves_b=1,levels=NULL")
        assert refused("max_leaves_a=2,d_levels_a=NULL", "NULL buffer of forest A") and refused("max_leaves_a=1,d_levels_new=NULL", "NULL output buffer")
        for case in ("n_trees_a=SIZE_MAX,n_trees_b=1", "n_trees_a=n_trees_b=SIZE_MAX/2+1", "n_pick*min(max_leaves_a,n_leaves_a)>SIZE_MAX/2",
                     "n_pick*min(max_leaves_b,n_leaves_b)>SIZE_MAX/2", "levels_cap=SIZE_MAX/64+1", "levels_cap=SIZE_MAX"):
            assert refused(case, "size overflow"), case
        assert not refused("n_pick*min(max_leaves_a,n_leaves_a)=SIZE_MAX/2", "size overflow") and not refused("levels_cap=SIZE_MAX/64", "size overflow")
        # the shape check's edges for each of the three forests: the value at the limit passes it, the one past it does not
        edges = [c for c in by if re.match(r"(A|B|new):", c)]
        assert len(edges) == 3 * 7
        for case in edges:
            past = case.endswith("+1") or ">SIZE_MAX/2" in case
            assert refused(case, "size overflow") == past, (case, by[case])
        for buf in SELECT_IN[:2] + ("d_roots_a",):
            assert refused(buf + "=NULL", "NULL buffer of forest A"), buf
        assert refused("d_levels_a=NULL", "NULL buffer of forest A") and refused("d_pick=NULL", "NULL d_pick")
        for buf in SELECT_IN[4:8]:
            assert refused(buf + "=NULL", "NULL buffer of forest B"), buf
        for buf in SELECT_OUT[:4]:
            assert refused(buf + "=NULL", "NULL output buffer"), buf
        assert accepted("d_n_bad=NULL")
        misaligned = [c for c in by if re.fullmatch(r"d_\w+\+\d", c)]
        assert len(misaligned) == 14 and all(refused(c, "aligned") for c in misaligned)
        # every output on the last bytes of every input and of every output before it; where the other ends, it is accepted
        n_in = n_out = 0
        for x, o in enumerate(SELECT_OUT):
            for i in SELECT_IN + SELECT_OUT[:x]:
                assert by["%s=%s+last" % (o, i)] == (-3, "merkle_forest_ragged_select: %s overlaps %s" % (o, i)), (o, i)
                assert accepted("%s=%s+end" % (o, i)), (o, i)
                n_in += i in SELECT_IN
                n_out += i in SELECT_OUT
        assert (n_in, n_out) == (45, 10)
        assert len([c for c in by if c.endswith("+last")]) == 55 and len([c for c in by if c.endswith("+end")]) == 55
        assert refused("d_roots_new=d_pick-16", "d_roots_new overlaps d_pick") and accepted("d_roots_new=d_pick-4*32")
        assert refused("d_leaves_new=d_leaves_b-leaves_cap*32+16", "d_leaves_new overlaps d_leaves_b") and accepted("d_leaves_new=d_leaves_b-leaves_cap*32")
        assert refused("d_leaves_new=d_levels_new", "d_levels_new overlaps d_leaves_new")
        assert refused("levels_cap=need+1,d_roots_new=d_levels_new+need*32", "d_roots_new overlaps d_levels_new") and accepted("d_roots_new=d_levels_new+need*32")


# ---- the kernels ----
@pytest.fixture(scope="module")
def compiled():
    return kernel_resources("forest_ragged.hip", os.path.join(CSRC, "_gen", "forest_select_test.s"))


def _kernel_bodies(isa):
    """{symbol: the text from its label to the end of its code} of every kernel of the listing"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", isa, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def test_select_kernels_meet_resource_targets(compiled):
    res, isa = compiled
    sel = {n: v for n, v in res.items() if "k_fr_sel_" in n}
    assert len(sel) >= 5, sorted(res)
    for want in ("k_fr_sel_sizes", "k_fr_sel_offsets", "k_fr_sel_tile_first", "k_fr_sel_move", "k_fr_sel_roots"):
        assert any(want in n for n in sel), want
    for name, v in sel.items():  # data movement and bookkeeping: no private memory, a quarter of the register file at the most
        assert v["scratch"] == 0 and v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)
    bodies = {n: b for n, b in _kernel_bodies(isa).items() if "k_fr_sel_" in n}
    assert len(bodies) == len(sel), (sorted(bodies), sorted(sel))
    for name, body in bodies.items():
        assert "scratch_" not in body, name
    # the build's own kernels are where they were
    assert len([n for n in res if "k_fr_digest" in n and "coop" not in n]) == 2
    assert len([n for n in res if "k_fr_digest_coop" in n]) == 2


def test_select_kernels_hash_nothing():
    import edgecases
    assert set(edgecases.hashing_kernels()) <= set(edgecases.named_kernels())
    src = open(os.path.join(CSRC, "forest_ragged.hip")).read()
    kernels = re.findall(r"__global__[^{;]*?\b(k_fr_sel_\w+)\s*\((.*?)\n}\n", src, flags=re.S)
    assert len(kernels) >= 5
    for name, body in kernels:
        for word in ("hades_permute", "node_digest_coop", "asm", "for (unsigned off = 1"):
            assert word not in body, (name, word)
    assert not re.search(r"\bk_fa_\w+\s*[(<]", src)  # the neighbour's kernels are not reached from here
    launcher = src[src.index("hipError_t launch_forest_select("):]
    assert launcher.count("launch_forest_ragged_index(") == 3 and "hipMemsetAsync" not in launcher and "hipMalloc" not in launcher


# ---- the Python methods ----
def _shapes(arity):
    D = {4: 2, 2: 4}[arity]  # depth of a tree of 9 .. 16 leaves
    return dict(n_a=16, t_a=2, m_a=9, n_b=24, t_b=3, m_b=12, n_pick=4, cap=30, D=D, lv_a=16 // (arity - 1) + 2 * D, lv_b=24 // (arity - 1) + 3 * D,
                lv_new=30 // (arity - 1) + 4 * D)


def _args(arity):
    s = _shapes(arity)
    return dict(a_leaves=dev(n=s["n_a"] * 4), a_off=dev(n=s["t_a"] + 1), a_lv=dev(n=s["lv_a"] * 4), a_roots=dev(n=s["t_a"] * 4),
                b_leaves=dev(n=s["n_b"] * 4), b_off=dev(n=s["t_b"] + 1), b_lv=dev(n=s["lv_b"] * 4), b_roots=dev(n=s["t_b"] * 4),
                d_pick=dev(n=s["n_pick"]), d_leaves_new=dev(n=s["cap"] * 4), d_offsets_new=dev(n=s["n_pick"] + 1), d_levels_new=dev(n=s["lv_new"] * 4 + 8),
                d_roots_new=dev(n=s["n_pick"] * 4), d_n_bad=dev(torch.int32))


def _call(method, a, s, with_b=True):
    fa = (a["a_leaves"], a["a_off"], s["t_a"], s["m_a"], a["a_lv"], a["a_roots"])
    fb = (a["b_leaves"], a["b_off"], s["t_b"], s["m_b"], a["b_lv"], a["b_roots"]) if with_b else None
    return method(fa, fb, a["d_pick"], s["n_pick"], a["d_leaves_new"], a["d_offsets_new"], a["d_levels_new"], a["d_roots_new"], a["d_n_bad"])


@pytest.mark.parametrize("arity", [4, 2])
def test_python_methods_refuse_bad_arguments_before_the_library(recorder, monkeypatch, arity):
    ctx = _no_device_context()
    s, args = _shapes(arity), _args(arity)
    method = ctx.merkle4_forest_ragged_select_device if arity == 4 else ctx.merkle2_forest_ragged_select_device
    symbol = "p252_merkle%d_forest_ragged_select_device_into" % arity
    _call(method, args, s)
    _call(method, args, s, with_b=False)
    assert recorder.calls == [symbol] * 2  # the control: the library is reached under this arity's symbol
    del recorder.calls[:]
    n_refused = 0
    for where, bad in with_cpu_tensor(args):
        with pytest.raises(ValueError, match="is on cpu"):
            _call(method, bad, s)
        assert recorder.calls == [], where
        n_refused += 1
    assert n_refused == 14
    # wrong element sizes
    for name, arg in (("a_off", "d_offsets_a"), ("b_off", "d_offsets_b"), ("d_pick", "d_pick"), ("d_offsets_new", "d_offsets_new")):
        with pytest.raises(ValueError, match=arg + " needs 8-byte elements"):
            _call(method, dict(args, **{name: dev(torch.int32)}), s)
    with pytest.raises(ValueError, match="d_n_bad needs 4-byte elements"):
        _call(method, dict(args, d_n_bad=dev()), s)
    # sizes one below what the call touches: the levels' cap one scalar below the bound, and every other buffer
    for name, arg, short in (("d_levels_new", "d_levels_new", dev(n=s["lv_new"] * 4 - 1)), ("a_off", "d_offsets_a", dev(n=s["t_a"])),
                             ("b_off", "d_offsets_b", dev(n=s["t_b"])), ("a_lv", "d_levels_a", dev(n=s["lv_a"] * 4 - 1)),
                             ("b_lv", "d_levels_b", dev(n=s["lv_b"] * 4 - 1)), ("a_roots", "d_roots_a", dev(n=s["t_a"] * 4 - 1)),
                             ("b_roots", "d_roots_b", dev(n=s["t_b"] * 4 - 1)), ("d_pick", "d_pick", dev(n=s["n_pick"] - 1)),
                             ("d_offsets_new", "d_offsets_new", dev(n=s["n_pick"])), ("d_roots_new", "d_roots_new", dev(n=s["n_pick"] * 4 - 1)),
                             ("d_leaves_new", "d_leaves_new", dev(n=3))):
        with pytest.raises(ValueError, match=arg + " holds"):
            _call(method, dict(args, **{name: short}), s)
    _call(method, dict(args, d_levels_new=dev(n=s["lv_new"] * 4)), s)  # the bound itself
    assert recorder.calls == [symbol]
    del recorder.calls[:]
    # overlapping buffers: an output inside an input, and two outputs in one buffer
    big = dev(n=4096)
    with pytest.raises(ValueError, match="d_leaves_new overlaps d_leaves_a"):
        _call(method, dict(args, a_leaves=big[:s["n_a"] * 4], d_leaves_new=big[s["n_a"] * 4 - 4:s["n_a"] * 4 - 4 + s["cap"] * 4]), s)
    with pytest.raises(ValueError, match="d_roots_new overlaps d_pick"):
        _call(method, dict(args, d_pick=big[:s["n_pick"]], d_roots_new=big[s["n_pick"] - 1:s["n_pick"] - 1 + s["n_pick"] * 4]), s)
    with pytest.raises(ValueError, match="d_levels_new overlaps d_leaves_new"):
        _call(method, dict(args, d_leaves_new=big[:s["cap"] * 4], d_levels_new=big[s["cap"] * 4 - 4:]), s)
    _call(method, dict(args, d_leaves_new=big[:s["cap"] * 4], d_levels_new=big[s["cap"] * 4:]), s)  # end to end: accepted
    assert recorder.calls == [symbol]
    del recorder.calls[:]
    assert "arity" not in __import__("inspect").signature(method).parameters
    from poseidon252_amd import merkle
    with pytest.raises(ValueError, match="arity"):
        merkle.forest_ragged_select(ctx, (args["a_leaves"], args["a_off"], s["t_a"], s["m_a"], args["a_lv"], args["a_roots"]), [0], arity=3)
    with pytest.raises(ValueError, match="forest_a"):
        method(None, None, args["d_pick"], 1, args["d_leaves_new"], args["d_offsets_new"], args["d_levels_new"], args["d_roots_new"])
    assert recorder.calls == []
    # the sizes the C call receives
    seen = []
    from poseidon252_amd import _lib
    real = _lib.lib().real

    class Spy:
        def __getattr__(self, name):
            if name == symbol:
                return lambda *a: seen.append(a) or 0
            return getattr(real, name)
    monkeypatch.setattr(_lib, "_lib", Spy())
    _call(method, args, s)
    _call(method, dict(args, d_n_bad=None), s, with_b=False)
    a, b = seen
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert a[1:] == (ptr(args["a_leaves"]), s["n_a"], ptr(args["a_off"]), s["t_a"], s["m_a"], ptr(args["a_lv"]), ptr(args["a_roots"]),
                     ptr(args["b_leaves"]), s["n_b"], ptr(args["b_off"]), s["t_b"], s["m_b"], ptr(args["b_lv"]), ptr(args["b_roots"]),
                     ptr(args["d_pick"]), s["n_pick"], ptr(args["d_leaves_new"]), s["cap"], ptr(args["d_offsets_new"]), ptr(args["d_levels_new"]),
                     s["lv_new"] + 2, ptr(args["d_roots_new"]), ptr(args["d_n_bad"]), 0)
    assert len(a) == N_ARGS and b[8:15] == (None, 0, None, 0, 0, None, None) and b[-2:] == (None, 0)


# ---- the model ----
def test_cap_rule_refuses_everything_non_empty_after_the_first_overflow():
    sizes = [5, 3, 1, 7, 2, 1]
    M = FS.select_model(4, sizes, [], [], [], [0, 1, 3, 2, 4, 9, 5], 9)
    # 5 + 3 = 8 fits; 7 takes the sum to 15 > 9; the one-leaf trees behind it would fit a greedy packer, and are refused all the same
    assert M["refused"] == [False, False, True, True, True, True, True] and M["n"] == [5, 3, 0, 0, 0, 0, 0] and M["n_bad"] == 5
    assert M["offsets_new"].tolist() == [0, 5, 8, 8, 8, 8, 8, 8]
    M = FS.select_model(4, sizes, [], [], [], [0, 1, 2], 9)  # the sum may reach the cap
    assert M["refused"] == [False] * 3 and M["offsets_new"].tolist() == [0, 5, 8, 9]
    # a bad tree and an id out of range bring nothing and do not move the sum
    M = FS.select_model(2, [5, 0, 3], [2], [4], [], [1, 2, 4, 0, 3], 9)
    assert M["refused"] == [True, True, True, False, False] and M["n"] == [0, 0, 0, 5, 4] and M["source"] == [0, 0, -1, 0, 1]


@pytest.mark.parametrize("arity", [4, 2])
def test_identity_pick_reproduces_the_source(arity):
    sizes = [1, 2, 3, arity, arity + 1, 63, 65, 1025, 16, 17]
    M = FS.select_model(arity, sizes, [], [], [], range(len(sizes)), sum(sizes))
    assert M["n"] == sizes and M["n_bad"] == 0
    assert M["offsets_new"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert np.array_equal(M["level_starts"], FS.level_starts_of(sizes, [], arity))
    from poseidon252_amd import _lib
    ll = _lib.lib().p252_merkle4_levels_len if arity == 4 else _lib.lib().p252_merkle2_levels_len
    assert [TS.levels_len(n, arity) for n in sizes] == [ll(n) for n in sizes]


@pytest.mark.parametrize("arity", [4, 2])
def test_duplicates_and_picks_from_b_land_where_levels_len_says(arity):
    sizes_a, sizes_b = [5, 1, 17], [64, 3]
    pick = [4, 0, 0, 3, 2, 1, 3]
    M = FS.select_model(arity, sizes_a, [], sizes_b, [], pick, 1000)
    want = [3, 5, 5, 64, 17, 1, 64]
    assert M["n"] == want and M["source"] == [1, 0, 0, 1, 0, 0, 1] and M["tree"] == [1, 0, 0, 0, 2, 1, 0]
    assert M["level_starts"].tolist() == np.concatenate([[0], np.cumsum([TS.levels_len(n, arity) for n in want])]).tolist()
    # the gather, on arrays whose values name their place
    def forest(sizes, base):
        n, lo = sum(sizes), FS.level_starts_of(sizes, [], arity)
        leaves = base + np.arange(n * 4, dtype=np.uint64).reshape(n, 4)
        levels = base + 100000 + np.arange(int(lo[-1]) * 4, dtype=np.uint64).reshape(-1, 4)
        roots = base + 200000 + np.arange(len(sizes) * 4, dtype=np.uint64).reshape(-1, 4)
        return leaves, np.concatenate([[0], np.cumsum(sizes)]), lo, levels, roots
    A, B = forest(sizes_a, 0), forest(sizes_b, 10 ** 6)
    leaves, levels, roots = FS.gather(M, arity, A, B)
    assert leaves.shape[0] == sum(want) and levels.shape[0] == int(M["level_starts"][-1]) and roots.shape[0] == len(pick)
    assert np.array_equal(leaves[:3], B[0][64:67]) and np.array_equal(leaves[3:8], A[0][:5]) and np.array_equal(leaves[8:13], A[0][:5])
    j = 4  # tree 2 of A
    lo = int(M["level_starts"][j])
    assert np.array_equal(levels[lo:lo + TS.levels_len(17, arity)], A[3][int(A[2][2]):int(A[2][3])])
    assert np.array_equal(roots[3], B[4][0]) and np.array_equal(roots[5], A[4][1])


def test_cpp_mirror_test_compiles(tmp_path, oracle_mod):
    build_cpp_mirror("test_forest_select_api", tmp_path)


def test_bench_tool_parses():
    bench_tool_parses("forest_select_bench", options=("--quick", "--reps", "--cases"))
