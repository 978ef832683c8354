"""Cases and exact checkers for the field primitives of csrc/fr29.hpp / hades29.hpp (entry points: csrc/primtest.hpp).

Plain Python big integers; shared by tests/test_primitives_cpu.py (host build), tests/test_primitives_gpu.py (the kernels)
and tests/test_host_arith.py::test_fold_top_quotient_bounds.  For every primitive: a generator that drives the inputs to the
ends of the range its header comment allows (and asserts that every case is inside it: nothing is filtered later), and a
checker of the congruence, the value range and the digit range the comment promises.  The figures are the headers' — never
what the code happens to return.  Seeds are fixed.

A case is (a, b, exp): a = the int32 inputs, b = the int64 inputs (strides: P252_PRIMTEST_LIST in primtest.hpp), exp = what
the checker needs (big integers).  At least N_MIN cases per primitive, at least a third of them constructed extremes.
"""
import random

import numpy as np

import pymodel

P = pymodel.P
NL, WB = 9, 29
DM = (1 << WB) - 1
TOPW = WB * (NL - 1)            # weight of the top digit: 2^232
RP = 1 << (WB * NL)             # R' = 2^261, as an integer
PINV = pow(P, -1, RP)
COL_LIMIT = 2 ** 63 - 2 ** 61   # fr29.hpp redc: "callers keep |column| < 2^63 - 2^61 before the call"
ROW_LIMIT = 2 ** 59             # fr29.hpp opaque_one: "Row columns stay below 2^59"
# row_redc1_lazy's own range (its comment): five one-digit products of un-carried lanes, |column| < 2^18.1 * 2^30.1; the
# digit step then adds its lo * p_k < 2^58 itself
LAZY_COL_LIMIT = int(2 ** 48.2)
LAZY_DIGIT = 2 ** 30.1          # "|d_k| < 2^30.1"
WIDE = 1 << 31                  # wide digits: a column's low register read as a signed number
N_MIN = 20000
N_RANDOM = 13000

HIST = 5


class ContractViolation(AssertionError):
    """a primitive returned something its header comment excludes: .prim and .clause say which and what"""

    def __init__(self, prim, clause, index, detail):
        super().__init__("%s: %s violated at case %d: %s" % (prim, clause, index, detail))
        self.prim, self.clause, self.index = prim, clause, index


# ---------------------------------------------------------------------------------------------------------------------
# digits
# ---------------------------------------------------------------------------------------------------------------------
def value(d):
    return sum(int(x) << (WB * k) for k, x in enumerate(d))


def carried(v):
    """digits 0..7 in [0, 2^29), the top digit signed"""
    d = []
    for _ in range(NL - 1):
        d.append(v & DM)
        v >>= WB
    assert -2 ** 31 <= v < 2 ** 31
    return d + [v]


def drifted(v, lim, push, rng):
    """the same value with digits 0..7 anywhere in [-lim, lim): push = +1 / -1 drives every digit to the positive / negative
    end of that range, 0 = random transfers between neighbours"""
    d = carried(v)
    for k in range(NL - 1):
        lo, hi = -((lim + d[k]) >> WB), (lim - 1 - d[k]) >> WB  # transfers that keep d[k] + t 2^29 inside [-lim, lim)
        t = {1: hi, -1: lo}.get(push, None)
        if t is None:
            t = rng.randint(lo, hi)
        d[k] += t << WB
        d[k + 1] -= t
    assert value(d) == v and all(-lim <= x < lim for x in d[:NL - 1]) and -2 ** 31 <= d[NL - 1] < 2 ** 31
    return d


def wide(v, push, rng):
    """wide digits (fr29.hpp redc_w<true>), |d| <= 2^31"""
    return drifted(v, WIDE, push, rng)


def low_digits_normal(prim, i, d):
    for k in range(NL - 1):
        if not 0 <= d[k] < (1 << WB):
            raise ContractViolation(prim, "digit range (digits 0..7 in [0, 2^29))", i, "digit %d = %d" % (k, d[k]))


def edge_values(lo, hi, per_edge):
    """integers strictly between lo and hi next to: both ends, 0, and every multiple of p in between"""
    anchors = [lo + 1, hi - 1, 0] + [k * P for k in range(lo // P, hi // P + 1)]
    seen, out = set(), []
    for a in anchors:
        for delta in range(per_edge):
            for v in (a - delta, a + delta):
                if lo < v < hi and v not in seen:
                    seen.add(v)
                    out.append(v)
    return out


def conv(cols, xd, yd):
    for i, xi in enumerate(xd):
        if xi:
            for j, yj in enumerate(yd):
                cols[i + j] += xi * yj


def balanced_const(rng, mag, mode):
    """nine constant digits with |g| <= mag: mode 0 all +mag, 1 all -mag, 2 alternating, 3 random signs at mag, 4 random"""
    if mode == 0:
        return [mag] * NL
    if mode == 1:
        return [-mag] * NL
    if mode == 2:
        return [mag if k % 2 == 0 else -mag for k in range(NL)]
    if mode == 3:
        return [rng.choice((mag, -mag)) for _ in range(NL)]
    return [rng.randint(-mag, mag) for _ in range(NL)]


class Cases:
    def __init__(self, prim, entry, check):
        self.prim, self.entry, self.check_one = prim, entry, check
        self.a, self.b, self.exp, self.n_extreme = [], [], [], 0

    def add(self, a, b, exp, extreme):
        self.a.append(a)
        self.b.append(b)
        self.exp.append(exp)
        self.n_extreme += bool(extreme)

    def __len__(self):
        return len(self.exp)

    def finish(self):
        n = len(self.exp)
        assert n >= N_MIN, (self.prim, n)
        assert 3 * self.n_extreme >= n, (self.prim, self.n_extreme, n)
        na, nb = len(self.a[0]), len(self.b[0])
        # (np.array raises on anything outside int32 / int64: an input that does not fit is a generator bug)
        self.a_arr = np.array(self.a, dtype=np.int32).reshape(n, na) if na else np.zeros((n, 0), dtype=np.int32)
        self.b_arr = np.array(self.b, dtype=np.int64).reshape(n, nb) if nb else np.zeros((n, 0), dtype=np.int64)
        self.a = self.b = None
        return self

    def check(self, out):
        """out: (n, stride) int32 as the primitive wrote it.  Raises ContractViolation on the first bad case; returns the worst
        observed figures (name -> float)."""
        rows = np.asarray(out).tolist()
        assert len(rows) == len(self.exp)
        worst = {}
        for i, (row, exp) in enumerate(zip(rows, self.exp)):
            for name, v in self.check_one(self.prim, i, row, exp):
                if v > worst.get(name, -1.0):
                    worst[name] = v
        return worst


def _words(v):
    return [(v >> (32 * k)) & 0xffffffff for k in range(8)]


def _u32(row):
    return [x & 0xffffffff for x in row]


# ---------------------------------------------------------------------------------------------------------------------
# to_mont4<5>, to_mont4<2>
# ---------------------------------------------------------------------------------------------------------------------
def _check_canonical(prim, i, row, v):
    got = _u32(row[:8])
    if got != _words(v % P):
        raise ContractViolation(prim, "value (limbs == V mod p, < p)", i, "V = %d p + %d: got %s" % (v // P, v % P, [hex(x) for x in got]))
    return ()


def gen_to_mont4(nsub, seed):
    """fr29.hpp to_mont4: 0 < V + 2p < (NSUB + 1) p; any int32 digits (the first pass carries in 64 bits)"""
    lo, hi = -2 * P, (nsub - 1) * P
    prim = "to_mont4<%d>" % nsub
    rng = random.Random(seed)
    cs = Cases(prim, "to_mont4_%d" % nsub, _check_canonical)

    def forms(v):
        return [carried(v), drifted(v, WIDE, 1, rng), drifted(v, WIDE, -1, rng), drifted(v, WIDE, 0, rng)]
    for v in edge_values(lo, hi, 160 if nsub == 5 else 340):
        for d in forms(v):
            cs.add(d, [], v, True)
    for _ in range(N_RANDOM // 2):
        v = rng.randrange(lo + 1, hi)
        assert lo < v < hi
        cs.add(carried(v), [], v, False)
        cs.add(drifted(v, rng.choice((1 << 30, WIDE)), 0, rng), [], v, False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# redc, redc_w<false|true>, mul_c_w<false|true>
# ---------------------------------------------------------------------------------------------------------------------
def _check_redc(prim, i, d, t):
    w = value(d)
    diff = t - w * RP
    if diff % P:
        raise ContractViolation(prim, "congruence (W 2^261 == T mod p)", i, "T = %d" % t)
    if not 0 <= diff < P * RP:
        raise ContractViolation(prim, "range (T/2^261 - p < W <= T/2^261)", i, "(T - W R')/(p R') = %.4f" % (diff / (P * RP)))
    low_digits_normal(prim, i, d)
    # (with the congruence the range leaves exactly one integer)
    assert w == (t - ((t * PINV) % RP) * P) // RP
    return (("(T/R' - W)/p", diff / (P * RP)), ("|top digit|", float(abs(d[NL - 1]))))


def _cols_ok(cols, limit=COL_LIMIT):
    assert all(abs(c) < limit for c in cols), max(abs(c) for c in cols)


def _tight_operands(rng, lim):
    """values with |x| < lim next to the ends, 0 and +-p, for products"""
    return [lim - 1, -(lim - 1), P, -P, 0, 1, -1, P + 1, P - 1, -P - 1, 1 - P, lim - 1 - rng.randrange(1 << 200), -(lim - 1) + rng.randrange(1 << 200)]


def gen_redc(seed=101):
    rng = random.Random(seed)
    cs = Cases("redc", "redc_t", _check_redc)
    lim = 2 * P

    def product(x, y, extreme):
        cols = [0] * (2 * NL)
        conv(cols, carried(x), carried(y))
        _cols_ok(cols)
        cs.add([], cols, x * y, extreme)

    def dot(xs, gs, extreme):
        cols = [0] * (2 * NL)
        for x, g in zip(xs, gs):
            conv(cols, carried(x), g)
        _cols_ok(cols)
        cs.add([], cols, sum(x * value(g) for x, g in zip(xs, gs)), extreme)
    edges = _tight_operands(rng, lim)
    for x in edges:
        for y in edges:
            product(x, y, True)
    ends = [lim - 1, -(lim - 1)]
    for k in range(3800):  # five-term dot products: operands at +-(2p - 1), constant digits all at +-2^28, every sign pattern
        xs = [ends[(k >> j) & 1] if k % 4 else ends[0] - rng.randrange(1 << 232) for j in range(5)]
        gs = [balanced_const(rng, 1 << 28, (k + j) % 4 if k % 3 else k % 4) for j in range(5)]
        dot(xs, gs, True)
    for k in range(3800):  # the same with the signs of x and g aligned digit by digit: every column as large as it gets
        gs = [balanced_const(rng, 1 << 28, k % 2) for _ in range(5)]
        xs = [(lim - 1 - rng.randrange(1 << (k % 250))) * (1 if k % 4 < 2 else -1) for _ in range(5)]
        dot(xs, gs, True)
    for _ in range(N_RANDOM // 2):
        product(rng.randrange(-lim + 1, lim), rng.randrange(-lim + 1, lim), False)
        dot([rng.randrange(-lim + 1, lim) for _ in range(5)], [balanced_const(rng, 1 << 28, 4) for _ in range(5)], False)
    return cs.finish()


def _check_redc_w(prim, i, d, t, wide_out=False):
    w = value(d)
    diff = w * RP - t
    if diff % P:
        raise ContractViolation(prim, "congruence (W 2^261 == T mod p)", i, "T = %d" % t)
    if not 100 * abs(diff) < 401 * P * RP:
        raise ContractViolation(prim, "range (|W - T/2^261| < 4.01 p)", i, "(W - T/R')/p = %.4f" % (diff / (P * RP)))
    if wide_out:
        for k in range(NL - 1):
            if not -WIDE <= d[k] < WIDE:
                raise ContractViolation(prim, "digit range (digits 0..7 in [-2^31, 2^31))", i, "digit %d = %d" % (k, d[k]))
    else:
        low_digits_normal(prim, i, d)
    return (("|W - T/R'|/p", abs(diff) / (P * RP)), ("|W|/p", abs(w) / P), ("max |digit 0..7|", float(max(abs(x) for x in d[:NL - 1]))),
            ("|top digit|", float(abs(d[NL - 1]))))


def _check_redc_w_wide(prim, i, d, t):
    return _check_redc_w(prim, i, d, t, True)


LAZY7 = 7 * P  # "the lazy range inside a permutation is |V| < 7p"


def gen_redc_w(wide_out, rows, seed):
    """T = one variable x variable product (carried digits, |x|, |y| up to 7p) or 1..5 variable x constant products with the
    variable in wide digits.  The constants' digits are bounded so that the documented column limit holds for the term count:
    n terms of nine products 2^31 |g| stay below 2^63 - 2^61 for |g| <= 2^28 / n (n = 1: the header's 9 x 2^59), and the
    actual table rows are used for one term (what the kernels do)."""
    rng = random.Random(seed)
    cs = Cases("redc_w<%s>" % ("true" if wide_out else "false"), "redc_w_wide" if wide_out else "redc_w_carried",
               _check_redc_w_wide if wide_out else _check_redc_w)
    lim = LAZY7

    def product(x, y, extreme):
        cols = [0] * (2 * NL)
        conv(cols, carried(x), carried(y))
        _cols_ok(cols)
        cs.add([], cols, x * y, extreme)

    def dot(xds, gs, extreme):
        cols = [0] * (2 * NL)
        for xd, g in zip(xds, gs):
            conv(cols, xd, g)
        _cols_ok(cols)
        cs.add([], cols, sum(value(xd) * value(g) for xd, g in zip(xds, gs)), extreme)
    edges = _tight_operands(rng, lim) + [2 * P, -2 * P, 6 * P + 1, -6 * P - 1]
    for x in edges:
        for y in edges:
            product(x, y, True)
    ends = [lim - 1, -(lim - 1)]
    for k in range(7200):
        n = 1 + k % 5
        mag = (1 << 28) // n
        push = 1 if (k // 5) % 2 == 0 else -1
        mode = (k // 10) % 4
        xds = [wide(ends[(k >> j) & 1] - (0 if k % 3 else rng.randrange(1 << 240)) * (1 if (k >> j) & 1 == 0 else -1), push, rng) for j in range(n)]
        dot(xds, [balanced_const(rng, mag, mode) for _ in range(n)], True)
    for k in range(len(rows)):  # every actual multiplier row against an operand pushed to either end
        for push in (1, -1):
            dot([wide(ends[k % 2], push, rng)], [rows[k]], True)
    for _ in range(N_RANDOM // 2):
        product(rng.randrange(-lim + 1, lim), rng.randrange(-lim + 1, lim), False)
        n = rng.randint(1, 5)
        dot([wide(rng.randrange(-lim + 1, lim), 0, rng) for _ in range(n)],
            [rng.choice(rows) if n == 1 and rng.random() < 0.5 else balanced_const(rng, (1 << 28) // n, 4) for _ in range(n)], False)
    return cs.finish()


def gen_mul_c_w(wide_out, rows, seed):
    """x carried and wide (|x| < 7p); n = the actual multiplier rows of the table and synthetic rows with every |g| = 2^28"""
    rng = random.Random(seed)
    cs = Cases("mul_c_w<%s>" % ("true" if wide_out else "false"), "mul_c_w_wide" if wide_out else "mul_c_w_carried",
               _check_redc_w_wide if wide_out else _check_redc_w)
    lim = LAZY7

    def one(xd, g, extreme):
        cols = [0] * (2 * NL)
        conv(cols, xd, g)
        _cols_ok(cols)
        assert abs(value(xd)) < lim and all(abs(x) <= 1 << 28 for x in g)
        cs.add(list(xd) + list(g), [], value(xd) * value(g), extreme)
    edges = edge_values(-lim, lim, 12)
    k = 0
    for v in edges:
        for form in range(3):
            xd = carried(v) if form == 0 else wide(v, 1 if form == 1 else -1, rng)
            one(xd, balanced_const(rng, 1 << 28, k % 4), True)
            one(xd, rows[k % len(rows)], True)
            k += 1
    while cs.n_extreme < 8000:
        v = (lim - 1 - rng.randrange(1 << 250)) * rng.choice((1, -1))
        one(wide(v, rng.choice((1, -1)), rng), balanced_const(rng, 1 << 28, k % 4), True)
        k += 1
    for _ in range(N_RANDOM):
        v = rng.randrange(-lim + 1, lim)
        xd = carried(v) if rng.random() < 0.3 else wide(v, 0, rng)
        one(xd, rng.choice(rows) if rng.random() < 0.6 else balanced_const(rng, 1 << 28, 4), False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# sbox, sbox_w<false|true>
# ---------------------------------------------------------------------------------------------------------------------
def _redc_exact(t):
    return (t - ((t * PINV) % RP) * P) // RP


def _check_sbox(prim, i, d, x):
    w = value(d)
    if (w * RP ** 4 - x ** 5) % P:
        raise ContractViolation(prim, "congruence (W 2^(4 x 261) == x^5 mod p)", i, "x = %d" % x)
    exp = _redc_exact(_redc_exact(_redc_exact(x * x) ** 2) * x)  # redc's range leaves one integer per step
    if w != exp:
        raise ContractViolation(prim, "range (each step in (T/2^261 - p, T/2^261])", i, "W/p = %.4f, expected %.4f" % (w / P, exp / P))
    low_digits_normal(prim, i, d)
    return (("|W|/p", abs(w) / P), ("|top digit|", float(abs(d[NL - 1]))))


def _check_sbox_w(prim, i, d, x, wide_out=False):
    w = value(d)
    if (w * RP ** 4 - x ** 5) % P:
        raise ContractViolation(prim, "congruence (W 2^(4 x 261) == x^5 mod p)", i, "x = %d" % x)
    if not 10 * abs(w) < 44 * P:
        raise ContractViolation(prim, "range (|W| < 4.4 p)", i, "W/p = %.4f" % (w / P))
    if wide_out:
        for k in range(NL - 1):
            if not -WIDE <= d[k] < WIDE:
                raise ContractViolation(prim, "digit range (digits 0..7 in [-2^31, 2^31))", i, "digit %d = %d" % (k, d[k]))
    else:
        low_digits_normal(prim, i, d)
    return (("|W|/p", abs(w) / P), ("max |digit 0..7|", float(max(abs(v) for v in d[:NL - 1]))), ("|top digit|", float(abs(d[NL - 1]))))


def _check_sbox_w_wide(prim, i, d, x):
    return _check_sbox_w(prim, i, d, x, True)


def gen_sbox(kind, seed):
    """kind: None = sbox (|x| < 2p), False / True = sbox_w<false|true> (|x| < 7p); x in carried digits, top digit of either sign"""
    rng = random.Random(seed)
    if kind is None:
        cs, lim = Cases("sbox", "sbox_t", _check_sbox), 2 * P
    else:
        cs = Cases("sbox_w<%s>" % ("true" if kind else "false"), "sbox_w_wide" if kind else "sbox_w_carried", _check_sbox_w_wide if kind else _check_sbox_w)
        lim = LAZY7
    for v in edge_values(-lim, lim, 300 if kind is None else 140):
        cs.add(carried(v), [], v, True)
    while cs.n_extreme < 8000:  # all digits at one end: 0 or 2^29 - 1, top digit at either end of the range
        top = rng.choice((lim >> TOPW, -(lim >> TOPW) - 1, 0, -1))
        d = [rng.choice((0, DM)) for _ in range(NL - 1)] + [top]
        v = value(d)
        if -lim < v < lim:
            cs.add(d, [], v, True)
    for _ in range(N_RANDOM):
        v = rng.randrange(-lim + 1, lim)
        cs.add(carried(v), [], v, False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# fold_top: the recurrence's shape, small_mul_add, arma_entry's U_1 row
# ---------------------------------------------------------------------------------------------------------------------
FOLD_TERM_LIMIT = int(5.3 * P)
FOLD_V_LIMIT = 1 << 283     # "|V| < 2^283"
COEF = pymodel.A_INT + pymodel.B_INT


def fold_top_recurrence_operands(wide_w, n, seed=5):
    """The nine terms of one step of the aligned recurrence at their extremes, for the actual coefficients: yields per trial the
    list of nine digit vectors (A_1..A_4 meet U values: carried digits; B_0..B_4 meet W values: wide digits when wide_w) and K's
    digits.  |term| up to 5.3 p; trial % 3 == 0: every term's sign and digit pushes WITH its coefficient's sign, == 1: value
    against and pushes with, == 2: random among +-limit and random values with random transfers."""
    rng = random.Random(seed)
    lim = FOLD_TERM_LIMIT
    n_a = len(pymodel.A_INT)
    for trial in range(n):
        terms = []
        for j, c in enumerate(COEF):
            if trial % 3 == 0:
                x, push = (lim if c > 0 else -lim), (1 if c > 0 else -1)
            elif trial % 3 == 1:
                x, push = (-lim if c > 0 else lim), (1 if c > 0 else -1)
            else:
                x, push = rng.choice([lim, -lim, rng.randrange(-lim, lim)]), 0
            terms.append(wide(x, push, rng) if (wide_w and j >= n_a) else carried(x))
        yield trial, terms, carried(rng.randrange(P))


def fold_top_recurrence_cols(wide_w, n, seed=5):
    for trial, terms, kd in fold_top_recurrence_operands(wide_w, n, seed):
        cols = list(kd)
        for dx, c in zip(terms, COEF):
            for k, d in enumerate(dx):
                cols[k] += d * c
        yield trial, cols


def _check_fold(prim, i, d, v):
    w = value(d)
    # (the range first: a quotient so far off that the top digit no longer fits its int32 is a range error before anything else)
    if not 10 * abs(w) < 12 * P:
        raise ContractViolation(prim, "range (|W| < 1.2 p)", i, "W/p = %.4f" % (w / P))
    if (w - v) % P:
        raise ContractViolation(prim, "congruence (W == V mod p)", i, "V = %d" % v)
    low_digits_normal(prim, i, d)
    return (("|W|/p", abs(w) / P), ("|top digit|", float(abs(d[NL - 1]))))


SBOX_W_OUT = int(4.4 * P)   # "all three stay below 4.4 p for |x| < 7p"


def _fold_cols_ok(cols):
    v = value(cols)
    assert abs(v) < FOLD_V_LIMIT
    _cols_ok(cols, 1 << 62)
    return v


def gen_fold_top(tab, lay, seed=7):
    rng = random.Random(seed)
    cs = Cases("fold_top", "fold_top_c", _check_fold)
    for wide_w in (False, True):
        for trial, cols in fold_top_recurrence_cols(wide_w, 12000, seed=5 + wide_w):
            cs.add([], cols, _fold_cols_ok(cols), trial % 3 != 2)
    # arma_entry's U_1 row: kappa + sum_j N[4][j] x_j, x = the S-box outputs of full round 3 (wide digits, below 4.4 p)
    n4 = tab[lay["INT_N"] + 4: lay["INT_N"] + 9]
    kap = tab[lay["AI_KAPPA"] + (3 * 5 + 4) * NL:][:NL]
    lim = SBOX_W_OUT
    for trial in range(9000):
        cols = list(kap)
        for j in range(5):
            if trial % 3 == 2:
                xd = wide(rng.randrange(-lim + 1, lim), 0, rng)
            else:
                s = 1 if (trial >> (2 + j)) & 1 == 0 or trial % 3 == 0 and trial % 2 == 0 else -1
                xd = wide(s * (lim - 1) - s * (rng.randrange(1 << 240) if trial % 6 >= 3 else 0), 1 if (trial >> 1) % 2 == 0 else -1, rng)
            for k in range(NL):
                cols[k] += xd[k] * n4[j]
        cs.add([], cols, _fold_cols_ok(cols), trial % 3 != 2)
    return cs.finish()


def gen_small_mul_add(tab, lay, seed=8):
    """W_0 = 28 X_4 + const: x = an S-box output (wide digits, below 4.4 p), the actual integer and row, and their negatives"""
    rng = random.Random(seed)
    cs = Cases("small_mul_add", "small_mul_add_x", _check_fold)
    m0 = lay["ENTRY_W0_INT"]
    add0 = tab[lay["AI_ENT_ADD"] + 3 * NL:][:NL]
    lim = SBOX_W_OUT

    def one(xd, m, add, extreme):
        cols = [xd[k] * m + add[k] for k in range(NL)]
        v = _fold_cols_ok(cols)
        assert v == value(xd) * m + value(add)
        cs.add(list(xd) + list(add) + [m], [], v, extreme)
    k = 0
    for v in edge_values(-lim, lim, 140):
        for push in (1, -1):
            m = (m0, -m0, 1, -1)[k % 4] if k % 5 == 0 else m0
            one(wide(v, push, rng), m, add0 if k % 7 else [-x for x in add0], True)
            k += 1
        one(carried(v), m0, add0, True)
    while cs.n_extreme < 8000:
        v = (lim - 1 - rng.randrange(1 << 250)) * rng.choice((1, -1))
        one(wide(v, rng.choice((1, -1)), rng), rng.choice((m0, -m0)), add0, True)
    for _ in range(N_RANDOM):
        one(wide(rng.randrange(-lim + 1, lim), 0, rng), rng.choice((m0, m0, -m0, 1, -1)), add0 if rng.random() < 0.7 else balanced_const(rng, 1 << 28, 4), False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# row_redc1, row_redc1_lazy
# ---------------------------------------------------------------------------------------------------------------------
def _check_row(prim, i, d, cols, lazy=False):
    t = value(cols)
    lo = cols[0] & DM
    w = value(d)
    if w << WB != t - lo * P:
        raise ContractViolation(prim, "value (W 2^29 == T - lo p)", i, "T = %d" % t)
    if not t - (P << WB) < w << WB <= t:
        raise ContractViolation(prim, "range (T/2^29 - p < W <= T/2^29)", i, "T = %d" % t)
    if lazy:
        for k in range(NL - 1):
            if not abs(d[k]) < LAZY_DIGIT:
                raise ContractViolation(prim, "digit range (|d_k| < 2^30.1)", i, "digit %d = %d" % (k, d[k]))
    else:
        low_digits_normal(prim, i, d)
    return (("max |digit 0..7| / 2^30", max(abs(x) for x in d[:NL - 1]) / 2.0 ** 30), ("|top digit|", float(abs(d[NL - 1]))))


def _check_row_lazy(prim, i, d, cols):
    return _check_row(prim, i, d, cols, True)


def gen_row(lazy, seed):
    """nine columns up to the limit the comment allows (row_redc1: 2^59; row_redc1_lazy: the 2^18.1 x 2^30.1 of its one caller —
    beyond that its un-carried digits leave the documented 2^30.1 by plain arithmetic), both signs"""
    rng = random.Random(seed)
    lim = LAZY_COL_LIMIT if lazy else ROW_LIMIT
    cs = Cases("row_redc1_lazy" if lazy else "row_redc1", "row_redc1_lazy_c" if lazy else "row_redc1_c", _check_row_lazy if lazy else _check_row)

    def one(cols, extreme):
        assert all(abs(c) < lim for c in cols)
        cs.add([], list(cols), list(cols), extreme)
    hi, lo = lim - 1, -(lim - 1)
    top = ((hi >> WB) - 1) << WB
    for pat in range(512):  # every sign pattern of columns at the limit
        one([hi if (pat >> k) & 1 else lo for k in range(NL)], True)
    for pat in range(512):  # the same with the low 29 bits of every column set / clear (lo = 2^29 - 1 / 0, carries at their ends)
        for low in (0, DM):
            one([(top if (pat >> k) & 1 else -top) + low for k in range(NL)], True)
    while cs.n_extreme < 8000:
        cols = [rng.choice((hi, lo, 0, hi - rng.randrange(1 << 29), lo + rng.randrange(1 << 29), DM, -DM, 1 << WB, -(1 << WB))) for _ in range(NL)]
        one(cols, True)
    for _ in range(N_RANDOM):
        one([rng.randrange(lo, hi + 1) for _ in range(NL)], False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# normalize, add_c, sub_e
# ---------------------------------------------------------------------------------------------------------------------
def _check_same_value(prim, i, d, v):
    if value(d) != v:
        raise ContractViolation(prim, "value (unchanged sum)", i, "expected %d, got %d" % (v, value(d)))
    low_digits_normal(prim, i, d)
    return (("|top digit|", float(abs(d[NL - 1]))),)


NORM_DIGIT = int(LAZY_DIGIT)  # what reaches normalize(): un-carried lanes of the integer layers, |d_k| < 2^30.1


def gen_normalize(seed=31):
    rng = random.Random(seed)
    cs = Cases("normalize", "normalize_x", _check_same_value)
    lim = LAZY7
    for v in edge_values(-lim, lim, 100):
        for push in (1, -1):
            cs.add(drifted(v, NORM_DIGIT, push, rng), [], v, True)
        cs.add(carried(v), [], v, True)
    while cs.n_extreme < 8000:  # every digit at one end of the range, either sign of the total
        d = [rng.choice((NORM_DIGIT - 1, -NORM_DIGIT, 0, DM, -1)) for _ in range(NL - 1)] + [rng.choice((0, -1, 1, -(1 << 26), 1 << 26))]
        cs.add(d, [], value(d), True)
    for _ in range(N_RANDOM):
        v = rng.randrange(-lim + 1, lim)
        cs.add(drifted(v, NORM_DIGIT, 0, rng), [], v, False)
    return cs.finish()


def gen_add_sub(sub, seed):
    """add_c: x a lazy residue in carried digits (|x| < 7p), c a constant row in balanced digits (|c_k| <= 2^28) or a scalar as
    from_mont4 loads it (digits in [0, 2^29), below 2^256); sub_e: x - y, both as from add_c's operands"""
    rng = random.Random(seed)
    cs = Cases("sub_e" if sub else "add_c", "sub_e_x" if sub else "add_c_x", _check_same_value)
    lim = LAZY7

    def one(xd, yd, extreme):
        cs.add(list(xd) + list(yd), [], value(xd) - value(yd) if sub else value(xd) + value(yd), extreme)
    loaded = [(1 << 256) - 1, 0, 1, P, P - 1, 2 * P, (1 << 256) - (1 << 232)]
    k = 0
    for v in edge_values(-lim, lim, 100):
        one(carried(v), carried(loaded[k % len(loaded)]), True)
        one(carried(v), balanced_const(rng, 1 << 28, k % 4), True)
        one(carried(v), carried(-loaded[k % len(loaded)] if sub else loaded[(k + 1) % len(loaded)]), True)
        k += 1
    while cs.n_extreme < 8000:  # digits all 0 / all 2^29 - 1 against each other: carries and borrows through the whole chain
        xd = [rng.choice((0, DM)) for _ in range(NL - 1)] + [rng.choice((0, -1, 1, (lim >> TOPW) - 1, -(lim >> TOPW)))]
        yd = [rng.choice((0, DM, 1)) for _ in range(NL - 1)] + [rng.choice((0, (1 << 24) - 1))]
        one(xd, yd, True)
    for _ in range(N_RANDOM):
        xd = carried(rng.randrange(-lim + 1, lim))
        one(xd, carried(rng.randrange(1 << 256)) if rng.random() < 0.5 else balanced_const(rng, 1 << 28, 4), False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# entry_row<1|2>, exit_row, ai_recur<QM>: the actual table rows
# ---------------------------------------------------------------------------------------------------------------------
WIDE_RANGE = int(5.2 * P)       # fr29.hpp E29: "< 5.2p after a wide one"; every consumer below takes at least this much
FOLD_OUT = int(1.2 * P)         # fold_top's output
W_TERM = int(4.1 * P)           # W_q = mul_c_w<true>(x^5, G_q): |x^5 G / R'| < 4.4 p x p/2 / 2^261 = 0.03 p, + 4.01 p


def _check_row_product(prim, i, d, exp):
    num, shift, fix, add = exp  # W == (num / 2^shift) fix / R' + add  (mod p)
    w = value(d)
    if ((w - add) * RP * (1 << shift) - num * fix) % P:
        raise ContractViolation(prim, "congruence (W == (sum n_j x_j / 2^(29 NDIG)) fix / 2^261 + add mod p)", i, "num = %d" % num)
    if not abs(w) < WIDE_RANGE:
        raise ContractViolation(prim, "range (|W| < 5.2 p, what sbox_w and the recurrence accept)", i, "W/p = %.4f" % (w / P))
    low_digits_normal(prim, i, d)
    return (("|W|/p", abs(w) / P), ("|top digit|", float(abs(d[NL - 1]))))


def gen_entry_row(ndig, tab, lay, seed):
    """x = the S-box outputs 0..3 of full round 3 (sbox_w<true>: wide digits, |x| < 4.4 p); rows 0, 1 (one digit) / 2 (two)"""
    rng = random.Random(seed)
    cs = Cases("entry_row<%d>" % ndig, "entry_row_%d" % ndig, _check_row_product)
    lim = SBOX_W_OUT
    rows = (0, 1) if ndig == 1 else (2,)
    for k in range(N_MIN + 1000):
        extreme = k < 9000
        r = rows[k % len(rows)]
        n = tab[lay["AI_ENT_N"] + r * NL:][:NL]
        fix = tab[lay["AI_ENT_FIX"] + r * NL:][:NL]
        add = tab[lay["AI_ENT_ADD"] + r * NL:][:NL]
        coef = [n[2 * j] + ((n[2 * j + 1] << WB) if ndig == 2 else 0) for j in range(4)]
        xs = []
        for j in range(5):
            if extreme:
                mode = (k // 2) % 4  # with the coefficient's sign, against it, sign pattern by bits of k, near the limit
                s = (1 if coef[j % 4] > 0 else -1) if mode == 0 else (-1 if coef[j % 4] > 0 else 1) if mode == 1 else (1 if (k >> (3 + j)) & 1 else -1)
                v = s * (lim - 1 - (rng.randrange(1 << 245) if mode == 3 else 0))
                push = s if (k // 8) % 2 == 0 else -s
            else:
                v, push = rng.randrange(-lim + 1, lim), 0
            assert abs(v) < lim
            xs.append(wide(v, push, rng))
        cols = [0] * (NL + ndig)
        for j in range(4):
            for kk in range(NL):
                cols[kk] += xs[j][kk] * n[2 * j]
                if ndig == 2:
                    cols[kk + 1] += xs[j][kk] * n[2 * j + 1]
        _cols_ok(cols, 1 << 62)
        num = sum(coef[j] * value(xs[j]) for j in range(4))
        cs.add([d for x in xs for d in x] + n + fix + add, [], (num, WB * ndig, value(fix), value(add)), extreme)
    return cs.finish()


def gen_exit_row(tab, lay, seed=43):
    """u = U_58..U_61 (fold_top outputs: carried digits, |U| < 1.2 p), w = W_57..W_60 (mul_c_w<true> outputs: wide digits)"""
    rng = random.Random(seed)
    cs = Cases("exit_row", "exit_row_x", _check_row_product)
    for k in range(N_MIN + 1000):
        extreme = k < 9000
        r = k % 4
        n = tab[lay["AI_EX_N"] + r * 2 * NL:][:2 * NL]
        fix = tab[lay["AI_EX_FIX"] + r * NL:][:NL]
        add = tab[lay["AI_EX_ADD"] + r * NL:][:NL]
        coef = [n[2 * t] + (n[2 * t + 1] << WB) for t in range(8)]
        ops = []
        for t in range(8):
            lim = FOLD_OUT if t < 4 else W_TERM
            if extreme:
                mode = (k // 4) % 4
                s = (1 if coef[t] > 0 else -1) if mode == 0 else (-1 if coef[t] > 0 else 1) if mode == 1 else (1 if (k >> (4 + t)) & 1 else -1)
                v = s * (lim - 1 - (rng.randrange(1 << 245) if mode == 3 else 0))
                push = s if (k // 16) % 2 == 0 else -s
            else:
                v, push = rng.randrange(-lim + 1, lim), 0
            assert abs(v) < lim
            ops.append(carried(v) if t < 4 else wide(v, push, rng))
        cols = [0] * (NL + 2)
        for t in range(8):
            for kk in range(NL):
                cols[kk] += ops[t][kk] * n[2 * t]
                cols[kk + 1] += ops[t][kk] * n[2 * t + 1]
        _cols_ok(cols, 1 << 62)
        num = sum(coef[t] * value(ops[t]) for t in range(8))
        cs.add([d for x in ops for d in x] + n + fix + add, [], (num, 2 * WB, value(fix), value(add)), extreme)
    return cs.finish()


def gen_ai_recur(qm, tab, lay, n, seed):
    """the rings as the step finds them: U_{q-j} at Us[(q - j) mod 5] (j = 0..3, carried digits), W_{q-j} at Ws[(q - j) mod 5]
    (j = 0..4, wide digits), terms up to 5.3 p at the extremes of fold_top_recurrence_operands; the slot the step overwrites holds
    a value it must not read; ab and K_{q+1} are the table's"""
    rng = random.Random(seed)
    cs = Cases("ai_recur<%d>" % qm, "ai_recur_%d" % qm, _check_fold)
    ab = tab[lay["AI_AB"]:][:NL]
    assert ab == COEF
    q5 = qm + HIST
    for trial, terms, _ in fold_top_recurrence_operands(True, n, seed):
        kg = tab[lay["AI_KG"] + (trial % 60) * 2 * NL:][:NL]
        us = [None] * HIST
        ws = [None] * HIST
        for j in range(4):
            us[(q5 - j) % HIST] = terms[j]
        us[(q5 + 1) % HIST] = wide(rng.choice((1, -1)) * (FOLD_TERM_LIMIT - 1), rng.choice((1, -1)), rng)  # (never read)
        for j in range(5):
            ws[(q5 - j) % HIST] = terms[4 + j]
        cols = list(kg)
        for dx, c in zip(terms, COEF):
            for k, d in enumerate(dx):
                cols[k] += d * c
        v = _fold_cols_ok(cols)
        cs.add([d for x in us + ws for d in x] + ab + kg, [], v, trial % 3 != 2)
    return cs


def finish_partial(cs_list, prim):
    """ai_recur's five instantiations are one primitive: the case counts are asserted over their sum"""
    n = sum(len(c) for c in cs_list)
    assert n >= N_MIN and 3 * sum(c.n_extreme for c in cs_list) >= n, prim
    for c in cs_list:
        na = len(c.a[0])
        c.a_arr = np.array(c.a, dtype=np.int32).reshape(len(c), na)
        c.b_arr = np.zeros((len(c), 0), dtype=np.int64)
        c.a = c.b = None
    return cs_list


# ---------------------------------------------------------------------------------------------------------------------
# store_output<false|true> (device only)
# ---------------------------------------------------------------------------------------------------------------------
R256_INV = pow(1 << 256, -1, P)
MASK250 = (1 << 250) - 1


def _check_store(prim, i, row, v):
    got = _u32(row)
    if got[:8] != _words(v % P):
        raise ContractViolation("store_output<false>", "value (BlsScalar limbs of V mod p)", i, "V = %d" % v)
    if got[8:] != _words(((v * R256_INV) % P) & MASK250):
        raise ContractViolation("store_output<true>", "value (raw limbs of (V 2^-256 mod p) & (2^250 - 1))", i, "V = %d" % v)
    return ()


def gen_store_output(seed=61):
    """any E29 with -2p < V < 2p in carried digits (what the tight reduction before the output stage leaves), top digit of either
    sign; among them every representative of the canonical values 0, 2^250 - 1, 2^250, 2^250 + 1 (the truncation's edge)"""
    rng = random.Random(seed)
    cs = Cases("store_output", "store_output", _check_store)
    lim = 2 * P
    for v in edge_values(-lim, lim, 900):
        cs.add(carried(v), [], v, True)
    for canon in [0, 1, (1 << 250) - 1, 1 << 250, (1 << 250) + 1, P - 1, MASK250 - 1] + [(1 << 250) + rng.randrange(-50, 50) for _ in range(300)]:
        v0 = (canon << 256) % P
        for v in (v0 - 2 * P, v0 - P, v0, v0 + P):
            if -lim < v < lim:
                assert ((v * R256_INV) % P) == canon % P
                cs.add(carried(v), [], v, True)
    for _ in range(N_RANDOM + 2000):
        v = rng.randrange(-lim + 1, lim)
        cs.add(carried(v), [], v, False)
    return cs.finish()


# ---------------------------------------------------------------------------------------------------------------------
# the dispatcher: primitive -> list of Cases (memoised: the CPU test, its UBSan child, the mutant control and the GPU test share them)
# ---------------------------------------------------------------------------------------------------------------------
def multiplier_rows(tab, lay):
    """every row of the table that multiplies a variable in a generic product of the kernels' schedule or the host cross-checks"""
    offs = [lay["AI_KG"] + (2 * q + 1) * NL for q in range(60)] + [lay["AI_ENT_FIX"] + i * NL for i in range(3)] + \
           [lay["AI_EX_FIX"] + i * NL for i in range(4)] + [lay["AI_F"], lay["INT_F"]] + [lay["INT_G"] + q * NL for q in range(60)]
    rows = [tab[o:o + NL] for o in offs]
    assert all(abs(x) <= 1 << 28 for r in rows for x in r)
    return rows


HOST_PRIMS = ["to_mont4<5>", "to_mont4<2>", "redc", "redc_w<false>", "redc_w<true>", "mul_c_w<false>", "mul_c_w<true>", "sbox", "sbox_w<false>",
              "sbox_w<true>", "fold_top", "small_mul_add", "row_redc1", "row_redc1_lazy", "normalize", "add_c", "sub_e", "entry_row<1>",
              "entry_row<2>", "exit_row", "ai_recur"]
DEVICE_ONLY_PRIMS = ["store_output"]
_memo = {}


def cases_for(prim, tab, lay):
    """list of Cases for one primitive (one element, except ai_recur: one per QM)"""
    if prim in _memo:
        return _memo[prim]
    rows = multiplier_rows(tab, lay)
    table = {
        "to_mont4<5>": lambda: [gen_to_mont4(5, 11)],
        "to_mont4<2>": lambda: [gen_to_mont4(2, 12)],
        "redc": lambda: [gen_redc()],
        "redc_w<false>": lambda: [gen_redc_w(False, rows, 13)],
        "redc_w<true>": lambda: [gen_redc_w(True, rows, 14)],
        "mul_c_w<false>": lambda: [gen_mul_c_w(False, rows, 15)],
        "mul_c_w<true>": lambda: [gen_mul_c_w(True, rows, 16)],
        "sbox": lambda: [gen_sbox(None, 17)],
        "sbox_w<false>": lambda: [gen_sbox(False, 18)],
        "sbox_w<true>": lambda: [gen_sbox(True, 19)],
        "fold_top": lambda: [gen_fold_top(tab, lay)],
        "small_mul_add": lambda: [gen_small_mul_add(tab, lay)],
        "row_redc1": lambda: [gen_row(False, 21)],
        "row_redc1_lazy": lambda: [gen_row(True, 22)],
        "normalize": lambda: [gen_normalize()],
        "add_c": lambda: [gen_add_sub(False, 32)],
        "sub_e": lambda: [gen_add_sub(True, 33)],
        "entry_row<1>": lambda: [gen_entry_row(1, tab, lay, 41)],
        "entry_row<2>": lambda: [gen_entry_row(2, tab, lay, 42)],
        "exit_row": lambda: [gen_exit_row(tab, lay)],
        "ai_recur": lambda: finish_partial([gen_ai_recur(qm, tab, lay, 4500, 50 + qm) for qm in range(HIST)], "ai_recur"),
        "store_output": lambda: [gen_store_output()],
    }
    _memo[prim] = table[prim]()
    return _memo[prim]


LAYOUT_NAMES = ["C_FIRST", "INT_N", "AI_AB", "AI_KAPPA", "AI_ENT_N", "AI_ENT_FIX", "AI_ENT_ADD", "AI_KG", "AI_EX_N", "AI_EX_FIX", "AI_EX_ADD",
                "AI_F", "INT_G", "INT_F", "ENTRY_W0_INT", "TOTAL"]
OUT_STRIDE = {"store_output": 16}


def out_stride(cs):
    return OUT_STRIDE.get(cs.entry, 8 if cs.entry.startswith("to_mont4") else NL)


def run_host(lib, cs):
    """one call of the host library's loop over all cases; returns the raw output rows"""
    import ctypes
    fn = getattr(lib, "pt_" + cs.entry)
    shape = (ctypes.c_int32 * 3)()
    getattr(lib, "pt_shape_" + cs.entry)(shape)
    assert list(shape) == [cs.a_arr.shape[1], cs.b_arr.shape[1], out_stride(cs)], (cs.entry, list(shape))
    out = np.full((len(cs), out_stride(cs)), 0x5a5a5a5a, dtype=np.int32)
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    a = np.ascontiguousarray(cs.a_arr) if cs.a_arr.size else np.zeros(1, dtype=np.int32)
    b = np.ascontiguousarray(cs.b_arr) if cs.b_arr.size else np.zeros(1, dtype=np.int64)
    fn(a.ctypes.data, b.ctypes.data, out.ctypes.data, len(cs))
    return out


def load_layout(lib):
    import ctypes
    v = (ctypes.c_int32 * len(LAYOUT_NAMES))()
    lib.pt_layout(v)
    return dict(zip(LAYOUT_NAMES, list(v)))


def load_table(hosttest_lib):
    import ctypes
    n = hosttest_lib.ht_tables29_total()
    t = np.zeros(n, dtype=np.int32)
    hosttest_lib.ht_tables29(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return t.tolist()


def format_worst(prim, worst):
    return "%-16s " % prim + ", ".join("%s %.4g" % (k, v) for k, v in sorted(worst.items()))


ENTRIES = ["to_mont4_5", "to_mont4_2", "redc_t", "redc_w_carried", "redc_w_wide", "mul_c_w_carried", "mul_c_w_wide", "sbox_t", "sbox_w_carried",
           "sbox_w_wide", "fold_top_c", "small_mul_add_x", "row_redc1_c", "row_redc1_lazy_c", "normalize_x", "add_c_x", "sub_e_x", "entry_row_1",
           "entry_row_2", "exit_row_x"] + ["ai_recur_%d" % qm for qm in range(HIST)]


def entry_names():
    """every entry of P252_PRIMTEST_LIST (primtest.hpp), plus the device-only output stage"""
    return ENTRIES + ["store_output"]


def main(argv):
    """python primcases.py <primtest host library> <hosttest library>: every host primitive's cases through that library (the
    UBSan build of tests/test_primitives_cpu.py runs in a process of its own: a trap ends the process)"""
    import ctypes
    lib, ht = ctypes.CDLL(argv[1]), ctypes.CDLL(argv[2])
    tab, lay = load_table(ht), load_layout(lib)
    for prim in HOST_PRIMS:
        for cs in cases_for(prim, tab, lay):
            print(format_worst(cs.prim, cs.check(run_host(lib, cs))))
        print("checked", prim, flush=True)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv))
