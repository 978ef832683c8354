// primtest.hpp — one entry point per field primitive of fr29.hpp / hades29.hpp, for tests only
// (tests/test_primitives_cpu.py, tests/test_primitives_gpu.py; the cases and the big-integer checkers are tests/primcases.py).
//
// Every entry has the same shape so that ONE dispatcher serves the host loops (primtest.cpp) and the device kernels
// (primtest.hip):   name(const int32_t* a, const int64_t* b, int32_t* out)
//   a   the case's int32 inputs (digits of the operands, constant rows, small integers), back to back
//   b   the case's int64 inputs (columns)
//   out what the primitive returned: nine raw digits, or the eight u32 words of the canonicalising ones
// Nothing is range-checked, carried or canonicalised in between: the tests see exactly what the primitive returns.
// P252_PRIMTEST_LIST(X) names every entry with its three strides: X(name, int32 in, int64 in, int32 out).
//
// Not part of the product: libposeidon252_hip.so contains none of these (tests/test_primitives_cpu.py asserts it).
#pragma once
#include "hades29.hpp"

namespace p252 {
namespace pt {

P252_HD E29 ld(const int32_t* a) {
    E29 e;
#pragma unroll
    for (int k = 0; k < NL; ++k) e.d[k] = a[k];
    return e;
}
P252_HD void st(int32_t* out, const E29& e) {
#pragma unroll
    for (int k = 0; k < NL; ++k) out[k] = e.d[k];
}
P252_HD void st_w(int32_t* out, const uint32_t w[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = (int32_t)w[k];
}

// ---- canonicalisation (a: x[9]) ----
P252_HD void to_mont4_5(const int32_t* a, const int64_t*, int32_t* out) {
    uint32_t w[8];
    to_mont4(ld(a), w);  // the DEFAULT number of conditional subtractions, as store_scalar asks for it
    st_w(out, w);
}
P252_HD void to_mont4_2(const int32_t* a, const int64_t*, int32_t* out) {
    uint32_t w[8];
    to_mont4<2>(ld(a), w);
    st_w(out, w);
}

// ---- full reductions (b: T[18]; the wide ones get acc_zero_w's bias first, so T excludes it) ----
P252_HD void redc_t(const int32_t*, const int64_t* b, int32_t* out) {
    A29 t;
#pragma unroll
    for (int k = 0; k < 2 * NL; ++k) t.c[k] = b[k];
    st(out, redc(t));
}
template <bool WIDE>
P252_HD void redc_w_any(const int64_t* b, int32_t* out) {
    const RK K = make_rk();
    A29 t;
    acc_zero_w<WIDE>(t, K);
#pragma unroll
    for (int k = 0; k < 2 * NL; ++k) t.c[k] += b[k];
    st(out, redc_w<WIDE>(t, K));
}
P252_HD void redc_w_carried(const int32_t*, const int64_t* b, int32_t* out) { redc_w_any<false>(b, out); }
P252_HD void redc_w_wide(const int32_t*, const int64_t* b, int32_t* out) { redc_w_any<true>(b, out); }

// ---- one generic product by a constant row (a: x[9], n[9]) ----
P252_HD void mul_c_w_carried(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    st(out, mul_c_w<false>(ld(a), a + NL, K));
}
P252_HD void mul_c_w_wide(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    st(out, mul_c_w<true>(ld(a), a + NL, K));
}

// ---- S-boxes (a: x[9]) ----
P252_HD void sbox_t(const int32_t* a, const int64_t*, int32_t* out) { st(out, sbox(ld(a))); }
P252_HD void sbox_w_carried(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    st(out, sbox_w<false>(ld(a), K));
}
P252_HD void sbox_w_wide(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    st(out, sbox_w<true>(ld(a), K));
}

// ---- reduction from the top (b: c[9]) and its small caller (a: x[9], add[9], m) ----
P252_HD void fold_top_c(const int32_t*, const int64_t* b, int32_t* out) {
    const RK K = make_rk();
    int64_t c[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) c[k] = b[k];
    st(out, fold_top(c, K));
}
P252_HD void small_mul_add_x(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    st(out, small_mul_add(ld(a), a[2 * NL], a + NL, K));
}

// ---- one-digit rows (b: c[9]) ----
P252_HD void row_redc1_c(const int32_t*, const int64_t* b, int32_t* out) {
    R29 t;
#pragma unroll
    for (int k = 0; k < NL; ++k) t.c[k] = b[k];
    st(out, row_redc1(t));
}
P252_HD void row_redc1_lazy_c(const int32_t*, const int64_t* b, int32_t* out) {
    R29 t;
#pragma unroll
    for (int k = 0; k < NL; ++k) t.c[k] = b[k];
    st(out, row_redc1_lazy(t));
}

// ---- digit-wise helpers (a: x[9] | x[9], c[9] | x[9], y[9]) ----
P252_HD void normalize_x(const int32_t* a, const int64_t*, int32_t* out) {
    E29 x = ld(a);
    normalize(x);
    st(out, x);
}
P252_HD void add_c_x(const int32_t* a, const int64_t*, int32_t* out) {
    E29 x = ld(a);
    add_c(x, a + NL);
    st(out, x);
}
P252_HD void sub_e_x(const int32_t* a, const int64_t*, int32_t* out) {
    E29 x = ld(a);
    sub_e(x, ld(a + NL));
    st(out, x);
}

// ---- the integer rows around the partial phase ----
// a: x[5][9], n[9], fix[9], add[9]
template <int NDIG>
P252_HD void entry_row_any(const int32_t* a, int32_t* out) {
    const RK K = make_rk();
    E29 x[WIDTH];
#pragma unroll
    for (int j = 0; j < WIDTH; ++j) x[j] = ld(a + j * NL);
    const int32_t* r = a + WIDTH * NL;
    st(out, entry_row<NDIG>(x, r, r + NL, r + 2 * NL, K));
}
P252_HD void entry_row_1(const int32_t* a, const int64_t*, int32_t* out) { entry_row_any<1>(a, out); }
P252_HD void entry_row_2(const int32_t* a, const int64_t*, int32_t* out) { entry_row_any<2>(a, out); }
// a: u[4][9], w[4][9], n[18], fix[9], add[9]
P252_HD void exit_row_x(const int32_t* a, const int64_t*, int32_t* out) {
    const RK K = make_rk();
    E29 u[4], w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        u[r] = ld(a + r * NL);
        w[r] = ld(a + (4 + r) * NL);
    }
    const E29* const up[4] = {&u[0], &u[1], &u[2], &u[3]};
    const E29* const wp[4] = {&w[0], &w[1], &w[2], &w[3]};
    const int32_t* r = a + 8 * NL;
    st(out, exit_row(up, wp, r, r + 2 * NL, r + 3 * NL, K));
}
// a: Us[5][9], Ws[5][9] (the rings as they lie), ab[9], kg[9]; out: the ring slot the step wrote, Us[(QM + 1) % HIST]
template <int QM>
P252_HD void ai_recur_any(const int32_t* a, int32_t* out) {
    const RK K = make_rk();
    E29 Us[HIST], Ws[HIST];
#pragma unroll
    for (int r = 0; r < HIST; ++r) {
        Us[r] = ld(a + r * NL);
        Ws[r] = ld(a + (HIST + r) * NL);
    }
    const int32_t* r = a + 2 * HIST * NL;
    ai_recur<QM>(Us, Ws, r, r + NL, K);
    st(out, Us[(QM + 1) % HIST]);
}
P252_HD void ai_recur_0(const int32_t* a, const int64_t*, int32_t* out) { ai_recur_any<0>(a, out); }
P252_HD void ai_recur_1(const int32_t* a, const int64_t*, int32_t* out) { ai_recur_any<1>(a, out); }
P252_HD void ai_recur_2(const int32_t* a, const int64_t*, int32_t* out) { ai_recur_any<2>(a, out); }
P252_HD void ai_recur_3(const int32_t* a, const int64_t*, int32_t* out) { ai_recur_any<3>(a, out); }
P252_HD void ai_recur_4(const int32_t* a, const int64_t*, int32_t* out) { ai_recur_any<4>(a, out); }

}  // namespace pt
}  // namespace p252

#define P252_PRIMTEST_LIST(X)      \
    X(to_mont4_5, 9, 0, 8)         \
    X(to_mont4_2, 9, 0, 8)         \
    X(redc_t, 0, 18, 9)            \
    X(redc_w_carried, 0, 18, 9)    \
    X(redc_w_wide, 0, 18, 9)       \
    X(mul_c_w_carried, 18, 0, 9)   \
    X(mul_c_w_wide, 18, 0, 9)      \
    X(sbox_t, 9, 0, 9)             \
    X(sbox_w_carried, 9, 0, 9)     \
    X(sbox_w_wide, 9, 0, 9)        \
    X(fold_top_c, 0, 9, 9)         \
    X(small_mul_add_x, 19, 0, 9)   \
    X(row_redc1_c, 0, 9, 9)        \
    X(row_redc1_lazy_c, 0, 9, 9)   \
    X(normalize_x, 9, 0, 9)        \
    X(add_c_x, 18, 0, 9)           \
    X(sub_e_x, 18, 0, 9)           \
    X(entry_row_1, 72, 0, 9)       \
    X(entry_row_2, 72, 0, 9)       \
    X(exit_row_x, 108, 0, 9)       \
    X(ai_recur_0, 108, 0, 9)       \
    X(ai_recur_1, 108, 0, 9)       \
    X(ai_recur_2, 108, 0, 9)       \
    X(ai_recur_3, 108, 0, 9)       \
    X(ai_recur_4, 108, 0, 9)
