"""Every field primitive of csrc/fr29.hpp / hades29.hpp, on its own, at the ends of the range its header comment allows
(csrc/primtest.hpp compiled for the host; cases and big-integer checkers: tests/primcases.py).

The whole-permutation tests feed these primitives effectively random values; a primitive that is wrong only next to the end of
its documented range would pass them.  Here each one gets its inputs constructed there, and the assertions are the documented
figures (1.2 p, 4.01 p, 4.4 p, [0, 2^29), ...), never the observed ones, which are only printed.  The same cases run again under
UBSan (signed overflow and shifts trap), and a control rebuilds the harness against headers with one subtle error each and
asserts that the checkers name the primitive and the clause."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

import primcases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def primtest_host():
    from poseidon252_amd import build as b
    return ctypes.CDLL(b.build_primtest_host())


@pytest.fixture(scope="module")
def table(hosttest_lib, primtest_host):
    """(the flat constant table the kernels read, where its rows lie)"""
    return pc.load_table(hosttest_lib), pc.load_layout(primtest_host)


@pytest.mark.parametrize("prim", pc.HOST_PRIMS)
def test_primitive_contract(prim, primtest_host, table):
    tab, lay = table
    for cs in pc.cases_for(prim, tab, lay):
        worst = cs.check(pc.run_host(primtest_host, cs))
        print(pc.format_worst(cs.prim, worst), "(%d cases, %d constructed extremes)" % (len(cs), cs.n_extreme))


def test_product_library_has_no_primitive_entry_points():
    """the harness is test-only: libposeidon252_hip.so gains no symbol"""
    from poseidon252_amd import build as b
    names = pc.entry_names()
    assert len(names) >= 25
    if shutil.which("nm") is None:  # (no binutils: ask the dynamic loader instead)
        L = ctypes.CDLL(b.LIB)
        assert not [e for e in names for sym in ("pt_" + e, "ptd_" + e, "pt_shape_" + e) if hasattr(L, sym)]
        return
    out = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for e in names:
        for sym in ("pt_" + e, "ptd_" + e, "pt_shape_" + e):
            assert sym not in exported, sym
    assert not [s for s in exported if s.startswith(("pt_", "ptd_", "k_pt_")) or "k_pt_" in s]


def test_primitive_contracts_under_ubsan(tmp_path, hosttest_lib):
    """the same cases against a build of primtest.cpp in which signed overflow and bad shifts abort: 'int64 columns cannot
    overflow' executed at the documented extremes, not only on the states a permutation happens to reach"""
    from poseidon252_amd import build as b
    so = str(tmp_path / "libp252_primtest_ubsan.so")
    subprocess.check_call(b.primtest_host_cmd(os.path.join(b.CSRC, "primtest.cpp"), so,
                                              extra=["-fsanitize=signed-integer-overflow,shift", "-fno-sanitize-recover=all"]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "primcases.py"), so, b.HOSTTEST_LIB], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count("checked ") == len(pc.HOST_PRIMS), r.stdout[-2000:]


# ---- the control: one textual edit per mutant, the primitive whose checker must object, and the clause it must name ----
_P2_OLD = """    const int32_t P2[NL] = {2 * P252_P29_0, 2 * P252_P29_1, 2 * P252_P29_2, 2 * P252_P29_3, 2 * P252_P29_4,
                            2 * P252_P29_5, 2 * P252_P29_6, 2 * P252_P29_7, 2 * P252_P29_8};"""
_REDC_TOP_OLD = """    r.d[NL - 1] = opaque_digit((int32_t)(t.c[2 * NL - 1] + carry));
    P252_TRK_TOP(r.d[NL - 1]);
    return r;
}

// ---- the wide Montgomery step"""
MUTANTS = [
    # (id, file, old, new, primitive, clause prefix)
    ("balanced_p_digit_5_plus_1", "fr29.hpp", "#define P252_PB_5 (201589969)", "#define P252_PB_5 (201589970)", "redc_w<false>", "congruence"),
    ("wstep_without_bias_xor", "fr29.hpp", "const int64_t q = opaque_digit((int32_t)((uint32_t)(c)[i] ^ 0x80000000u));",
     "const int64_t q = opaque_digit((int32_t)((uint32_t)(c)[i]));", "redc_w<false>", "congruence"),
    ("last_wide_digit_carry_dropped", "fr29.hpp", "            t.c[NL + k + 1] += h * (int64_t)K.eight;",
     "            if (k < NL - 2) t.c[NL + k + 1] += h * (int64_t)K.eight;", "redc_w<true>", "congruence"),
    ("fold_shift_19", "fr29.hpp", "#define P252_FOLD_SHIFT 20", "#define P252_FOLD_SHIFT 19", "fold_top", "range"),
    ("to_mont4_default_nsub_4", "fr29.hpp", "template <int NSUB = 5>", "template <int NSUB = 4>", "to_mont4<5>", "value"),
    ("to_mont4_offset_one_p", "fr29.hpp", _P2_OLD, _P2_OLD.replace("2 * P252_P29_", "1 * P252_P29_"), "to_mont4<5>", "value"),
    ("lazy_row_without_carry_in", "fr29.hpp", " + (int32_t)(t.c[k] >> WB));", ");", "row_redc1_lazy", "value"),
    ("acc_sqr_first_cross_term_not_doubled", "fr29.hpp", "for (int j = i + 1; j < NL; ++j) t.c[i + j] += a2 * (int64_t)a.d[j];",
     "for (int j = i + 1; j < NL; ++j) t.c[i + j] += (j == i + 1 ? (int64_t)a.d[i] : a2) * (int64_t)a.d[j];", "sbox", "congruence"),
    ("redc_top_digit_without_carry", "fr29.hpp", _REDC_TOP_OLD, _REDC_TOP_OLD.replace("[2 * NL - 1] + carry));", "[2 * NL - 1]));"), "redc", "congruence"),
]
# further primitives every mutant must ALSO be caught in, where the edit sits in code they share (a hole there is a hole in primcases.py)
ALSO = {
    "balanced_p_digit_5_plus_1": ["redc_w<true>", "fold_top", "mul_c_w<false>", "sbox_w<true>", "exit_row", "ai_recur"],
    "wstep_without_bias_xor": ["redc_w<true>", "mul_c_w<true>", "sbox_w<false>", "entry_row<1>", "entry_row<2>", "exit_row"],
    "last_wide_digit_carry_dropped": ["mul_c_w<true>", "sbox_w<true>"],
    "fold_shift_19": ["small_mul_add", "ai_recur"],
    "to_mont4_offset_one_p": ["to_mont4<2>"],
    "acc_sqr_first_cross_term_not_doubled": ["sbox_w<false>", "sbox_w<true>"],
}


def _first_violation(lib, prim, tab, lay):
    for cs in pc.cases_for(prim, tab, lay):
        try:
            cs.check(pc.run_host(lib, cs))
        except pc.ContractViolation as e:
            return e
    return None


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_primitive_tests_kill_mutants(mutant, tmp_path, table, primtest_host):
    """CPU only: a copy of the headers with ONE subtle error, the harness rebuilt against it, and the checkers must report the
    named primitive and clause.  (The unmutated build passes the same checkers: test_primitive_contract.)"""
    from poseidon252_amd import build as b
    name, fname, old, new, prim, clause = mutant
    tab, lay = table
    for f in b.PRIMTEST_HOST_SOURCES:
        shutil.copy(os.path.join(b.CSRC, f), str(tmp_path / f))
    src = (tmp_path / fname).read_text()
    assert src.count(old) == 1, "%s: the edit must match exactly once, matched %d times" % (name, src.count(old))
    assert old != new
    (tmp_path / fname).write_text(src.replace(old, new))
    so = str(tmp_path / ("libp252_primtest_%s.so" % name))
    subprocess.check_call(b.primtest_host_cmd(str(tmp_path / "primtest.cpp"), so, extra=["-O1"]))
    lib = ctypes.CDLL(so)
    for target in [prim] + ALSO.get(name, []):
        e = _first_violation(lib, target, tab, lay)
        assert e is not None, "mutant %s survives the checks of %s" % (name, target)
        assert e.prim.startswith(target.split("<")[0]) and str(e).startswith(e.prim), str(e)
        if target == prim:
            assert e.prim == prim or prim == "ai_recur", str(e)
            assert e.clause.startswith(clause), "mutant %s: expected the %s clause of %s, got: %s" % (name, clause, prim, e)
        print("%s killed by %s" % (name, e))
    # the control of the control: the unmutated sources, built the same way, pass the same checkers
    if name == MUTANTS[0][0]:
        (tmp_path / fname).write_text(src)
        so0 = str(tmp_path / "libp252_primtest_plain.so")
        subprocess.check_call(b.primtest_host_cmd(str(tmp_path / "primtest.cpp"), so0, extra=["-O1"]))
        assert _first_violation(ctypes.CDLL(so0), prim, tab, lay) is None
