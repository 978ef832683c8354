// fr29.hpp — BLS12-381 scalar-field arithmetic for gfx950 VALU: 9 x 29-bit limbs, 64-bit columns.
//
// Replaces, for batched GPU use, the BlsScalar operations the reference calls at
// src/hades/permutation/scalar.rs:34 (add), :47 (+=), :51 (square, mul), :59 (mul, +=).
//
// Why this shape (measured, profiles/r01_valu_rates_gfx950.txt): on gfx950 v_mad_u64_u32 /
// v_mad_i64_i32 issue at the same 4-cycle-per-wave rate as v_fma_f64, and v_add_co/v_addc carry
// instructions cost exactly as much as a multiply-add.  Saturated 32-bit limbs would spend one carry
// instruction per product; 29-bit limbs leave 6 bits of headroom per product so that a whole
// 5-term dot product (45 products per column) accumulates in a 64-bit column with NO carry
// instructions at all, and is Montgomery-reduced once.
//
// Representation ("E29"): value V = sum d[i] * 2^(29 i), d[0..7] in [0, 2^29), d[8] signed and small.
// V is a LAZY residue (|V| < 2p after a tight reduction, < 5.2p after a wide one — redc_w below): at the kernels' boundary any integer congruent to x*R (R = 2^256, the
// reference's Montgomery radix); inside a permutation congruent to s*x for a known per-round scale s
// (tables.hpp).  Signs are tolerated everywhere (columns are signed 64-bit, multiplier constants
// are balanced digits in [-2^28, 2^28]); only to_mont4() canonicalises to [0, p).
//
// Montgomery reduction here divides by R' = 2^261 (9 digits), not by R, and one-digit rows divide by
// 2^29 per digit step.  Powers of two never cost anything: they are folded into the constant tables /
// the scale of the stored values.
//
// All functions are __host__ __device__: the same code is unit-tested on the CPU against the
// oracle (tests/test_host_arith.py) and runs in the kernels.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P252_HD __host__ __device__ __forceinline__
#else
#define P252_HD inline __attribute__((always_inline))
#endif

namespace p252 {

constexpr int NL = 9;                       // digits per element
constexpr int WB = 29;                      // bits per digit
constexpr uint32_t DMASK = (1u << WB) - 1;  // 0x1fffffff

// p = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 in radix 2^29.
// p[0] == 1  =>  -p^{-1} mod 2^29 == 2^29 - 1  =>  the Montgomery quotient digit is just -t mod 2^29.
#define P252_P29_0 0x00000001
#define P252_P29_1 0x1ffffff8
#define P252_P29_2 0x1f96ffbf
#define P252_P29_3 0x1b4805ff
#define P252_P29_4 0x1d80553b
#define P252_P29_5 0x0c0404d0
#define P252_P29_6 0x1520cce7
#define P252_P29_7 0x0a6533af
#define P252_P29_8 0x0073eda7

struct E29 {
    int32_t d[NL];
};

// Instrumented host build only (tests/test_host_arith.py::test_dynamic_bounds): largest |column| any reduction saw and
// largest |top digit| any reduction produced.  Compiles to nothing everywhere else.
#if defined(P252_TRACK_BOUNDS) && !defined(__HIPCC__)
struct BoundTrack {
    int64_t max_col = 0;
    int32_t max_top = 0;   // reduction outputs (multiplicands of generic products)
    int32_t max_top1 = 0;  // W_0 = 28 X_4 + const (multiplicand of one-digit products only)
};
inline BoundTrack& bound_track() {  // per thread (the cooperative digest's host test runs eight of them and merges)
    static thread_local BoundTrack b;
    return b;
}
inline void trk_col(int64_t v) {
    if (v < 0) v = -(v + 1);
    if (v > bound_track().max_col) bound_track().max_col = v;
}
inline void trk_top(int32_t d) {
    if (d < 0) d = -(d + 1);
    if (d > bound_track().max_top) bound_track().max_top = d;
}
#define P252_TRK_COL(v) trk_col(v)
#define P252_TRK_TOP(d) trk_top(d)
#define P252_TRK_TOP1(d)                                                        \
    {                                                                           \
        int32_t a_ = (d) < 0 ? -((d) + 1) : (d);                                \
        if (a_ > bound_track().max_top1) bound_track().max_top1 = a_;           \
    }
#else
#define P252_TRK_TOP1(d)
#define P252_TRK_COL(v)
#define P252_TRK_TOP(d)
#endif

// Hides the value range of a freshly masked digit from the optimiser.  Without it LLVM knows the
// digit is non-negative, treats (int64)digit * (int64)signed_constant as zext x sext and lowers it to
// TWO v_mad_u64_u32 plus two v_mov (unsigned product + sign correction) instead of ONE
// v_mad_i64_i32 — measured: 1,200 of 3,050 instructions per partial round.  Emits no instruction.
P252_HD int32_t opaque_digit(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}

// Keeps the instruction scheduler from interleaving two large independent computations (e.g. successive rows of
// the exit): interleaving buys no throughput here (the issue slots are full either way) but it keeps both
// accumulator sets live, and the sponge-type kernels then exceed 256 VGPRs = drop to one wave per SIMD.
P252_HD void sched_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// 18 signed 64-bit columns: column k has weight 2^(29 k).
struct A29 {
    int64_t c[2 * NL];
};

P252_HD void acc_zero(A29& t) {
#pragma unroll
    for (int k = 0; k < 2 * NL; ++k) t.c[k] = 0;
}

// t = x * R'  (x placed in the high columns): after redc it contributes exactly x.
P252_HD void acc_set_hi(A29& t, const E29& x) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        t.c[k] = 0;
        t.c[NL + k] = x.d[k];
    }
}
template <class CP>
P252_HD void acc_set_hi_c(A29& t, CP c) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        t.c[k] = 0;
        t.c[NL + k] = c[k];
    }
}
// t += a * b, b = 9 digits readable as b[j] (constant-table pointer or E29::d)
template <class BP>
P252_HD void acc_mul(A29& t, const E29& a, BP b) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int64_t bj = b[j];
#pragma unroll
        for (int i = 0; i < NL; ++i) t.c[i + j] += (int64_t)a.d[i] * bj;
    }
}

// 2 x as an ADD: on gfx950 v_add_u32 issues at the 2-cycle rate, v_lshlrev_b32 (what x * 2 compiles to) at the 4-cycle
// rate (profiles/r02_valu_rates_gfx950.txt) — 1,600 doublings per permutation.
P252_HD int32_t twice(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x * 2;
#endif
}

// t += a * a  (45 products instead of 81)
P252_HD void acc_sqr(A29& t, const E29& a) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        t.c[2 * i] += (int64_t)a.d[i] * (int64_t)a.d[i];
        const int64_t a2 = (int64_t)twice(a.d[i]);  // |d| < 2^29 -> fits int32
#pragma unroll
        for (int j = i + 1; j < NL; ++j) t.c[i + j] += a2 * (int64_t)a.d[j];
    }
}

// Montgomery reduction by R' = 2^261, digit-serial, with a NEGATIVE quotient digit: step i subtracts
// lo_i * p * 2^(29 i) where lo_i = t_i mod 2^29 (p[0] == 1, so column i becomes t_i - lo_i, an exact
// multiple of 2^29 whose quotient is simply t_i >> 29 — no add, no negate, no zero-extension).
// Returns V' = (T - m p) / 2^261 with 0 <= m < 2^261, i.e. V' in (T/R' - p, T/R'].
// Cost per step: 1 v_and + 8 v_mad_i64_i32 + 1 v_ashrrev_i64 + 1 v_lshl_add_u64.
// Column bound: callers keep |column| < 2^63 - 2^61 before the call (see DESIGN.md "bounds").
P252_HD E29 redc(A29& t) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        P252_TRK_COL(t.c[i]);
        const int64_t lo = opaque_digit((int32_t)((uint32_t)t.c[i] & DMASK));
        t.c[i + 1] += (t.c[i] >> WB) - lo * (int64_t)P252_P29_1;
        t.c[i + 2] -= lo * (int64_t)P252_P29_2;
        t.c[i + 3] -= lo * (int64_t)P252_P29_3;
        t.c[i + 4] -= lo * (int64_t)P252_P29_4;
        t.c[i + 5] -= lo * (int64_t)P252_P29_5;
        t.c[i + 6] -= lo * (int64_t)P252_P29_6;
        t.c[i + 7] -= lo * (int64_t)P252_P29_7;
        t.c[i + 8] -= lo * (int64_t)P252_P29_8;
    }
    E29 r;
    int64_t carry = 0;
#pragma unroll
    for (int k = 0; k < NL - 1; ++k) {
        const int64_t v = t.c[NL + k] + carry;
        P252_TRK_COL(t.c[NL + k]);
        r.d[k] = opaque_digit((int32_t)((uint32_t)v & DMASK));
        carry = v >> WB;
    }
    P252_TRK_COL(t.c[2 * NL - 1] + carry);
    r.d[NL - 1] = opaque_digit((int32_t)(t.c[2 * NL - 1] + carry));
    P252_TRK_TOP(r.d[NL - 1]);
    return r;
}

// ---- the wide Montgomery step (kernels' schedule) ----
// p = 1 - 2^32 + ... : p == 1 (mod 2^32), not only (mod 2^29).  Take the quotient digit from ALL 32 bits of the column's
// low register instead of its low 29: q == column (mod 2^32), q in [-2^31, 2^31).  Then column - q is an exact multiple
// of 2^32, so the carry into the next column, (column - q) / 2^29, is 8 x (the column's HIGH REGISTER): one
// v_mad_i64_i32 with the constant 8 does sign extension, shift and add, where the 29-bit step needs v_and + v_ashrrev_i64
// + v_lshl_add_u64 (2 + 4 + 4 cycles).  To read q as a signed number without a correction term the columns that get a
// step carry a bias of 2^31 (set when the accumulator is initialised — the first multiply-add of a column takes it
// as its addend, a register pair that lives for the whole kernel): u = low register of (column + 2^31);
// q = u XOR 2^31 = u - 2^31; (column - q) / 2^32 = high register, exactly.  Cost per step: 1 v_xor + 9 v_mad_i64_i32.
// Multiples of p are subtracted in BALANCED digits (|p'_k| < 2^28, sum |p'_k| = 2^29.37 where the plain digits sum to
// 2^31.36), so a column collects less than 2^31 x 2^29.37 = 2^60.4 from a whole reduction although q has 32 bits.
// Result: V' = (T - m p) / 2^(29 n) with |m| < 2^(29 n + 2)  =>  V' in (T/2^(29 n) - 4.01 p, T/2^(29 n) + 4.01 p): the lazy
// range inside a permutation is |V| < 7p (top digit < 2^26) instead of < 2p; only the LAST reduction before to_mont4()
// must be the tight one (redc).
#define P252_PB_1 (-8) /* = -RK::eight: the step multiplies by the register constant */
#define P252_PB_2 (-6881344)
#define P252_PB_3 (-79165952)
#define P252_PB_4 (-41921220)
#define P252_PB_5 (201589969)
#define P252_PB_6 (-182399769)
#define P252_PB_7 (174404528)
#define P252_PB_8 (7597479)

// reduction constants that live in registers for a whole kernel (made once, passed down by reference)
struct RK {
    int64_t bias;   // 2^31, a VGPR pair: the addend of the first multiply-add of every column that gets a wide step
    int32_t eight;  // 8, an SGPR the optimiser cannot see through (so that x8 stays a multiply-add, not shift + add)
    int32_t eight_p1;  // -p'_1 = 8 again, a second opaque copy: with one, h*8 + q*8 is refactored into a 64-bit (h+q)*8
    int32_t neg1;      // -1 = -p'_0 for fold_top: column 0 -= q as ONE multiply-add instead of a two-instruction 64-bit subtract
};
P252_HD RK make_rk() {
    RK k;
    k.bias = (int64_t)1 << 31;
    k.eight = 8;
    k.eight_p1 = 8;
    k.neg1 = -1;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(k.bias));
    asm("; carry x8" : "+s"(k.eight));  // (distinct strings: identical asm statements would be merged)
    asm("; -p'_1" : "+s"(k.eight_p1));
    asm("; -p'_0" : "+s"(k.neg1));
#endif
    return k;
}

// one wide step on a column array: c[i] carries the bias; c[i+1] .. c[i+8] (as far as NCOL goes) receive -q p'_k
#define P252_WSTEP(c, i, NCOL, K)                                                         \
    {                                                                                     \
        P252_TRK_COL((c)[i]);                                                             \
        const int64_t q = opaque_digit((int32_t)((uint32_t)(c)[i] ^ 0x80000000u));        \
        const int64_t h = (int32_t)((c)[i] >> 32);                                        \
        (c)[(i) + 1] += h * (int64_t)(K).eight + q * (int64_t)(K).eight_p1; /* p'_1 = -8 */ \
        if ((i) + 2 < (NCOL)) (c)[(i) + 2] -= q * (int64_t)P252_PB_2;                     \
        if ((i) + 3 < (NCOL)) (c)[(i) + 3] -= q * (int64_t)P252_PB_3;                     \
        if ((i) + 4 < (NCOL)) (c)[(i) + 4] -= q * (int64_t)P252_PB_4;                     \
        if ((i) + 5 < (NCOL)) (c)[(i) + 5] -= q * (int64_t)P252_PB_5;                     \
        if ((i) + 6 < (NCOL)) (c)[(i) + 6] -= q * (int64_t)P252_PB_6;                     \
        if ((i) + 7 < (NCOL)) (c)[(i) + 7] -= q * (int64_t)P252_PB_7;                     \
        if ((i) + 8 < (NCOL)) (c)[(i) + 8] -= q * (int64_t)P252_PB_8;                     \
    }

// accumulator for a product that will be reduced by redc_w: bias in the nine low columns; WIDE (the result leaves as
// wide digits, see redc_w): in the high columns 9..16 as well
template <bool WIDE = false>
P252_HD void acc_zero_w(A29& t, const RK& K) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        t.c[k] = K.bias;
        t.c[NL + k] = (WIDE && k < NL - 1) ? K.bias : (int64_t)0;
    }
}
template <class CP>
P252_HD void acc_set_hi_c_w(A29& t, CP c, const RK& K) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        t.c[k] = K.bias;
        t.c[NL + k] = c[k];
    }
}

// nine wide steps + the carry chain over the high columns (digits 0..7 in [0, 2^29), top digit signed, |top| < 2^26).
// WIDE = true: the result leaves as WIDE DIGITS instead — digit k = the whole low register of column 9 + k read as a signed
// number (the bias trick of the wide step again: q = low register XOR 2^31, the rest of the column, 8 x its high register,
// goes to the next column), |digit| <= 2^31: 2 instructions and 6 issue cycles per digit where the carry chain takes 3 and
// 10.  Such a value may only be a MULTIPLICAND OF CONSTANTS — a generic product by balanced constant digits (|g| <= 2^28:
// columns stay below 9 x 2^59 + 2^60.4) or one- / two-digit integer rows — never of another variable: the S-box outputs
// of the full rounds (-> integer rows), x^5 of a partial round (-> G) and W_q (-> the recurrence, the exit rows).
// tables.hpp max_column_bound29 charges 2^31 per digit for exactly those operands.
template <bool WIDE = false>
P252_HD E29 redc_w(A29& t, const RK& K) {
    P252_WSTEP(t.c, 0, 2 * NL, K)
    P252_WSTEP(t.c, 1, 2 * NL, K)
    P252_WSTEP(t.c, 2, 2 * NL, K)
    P252_WSTEP(t.c, 3, 2 * NL, K)
    P252_WSTEP(t.c, 4, 2 * NL, K)
    P252_WSTEP(t.c, 5, 2 * NL, K)
    P252_WSTEP(t.c, 6, 2 * NL, K)
    P252_WSTEP(t.c, 7, 2 * NL, K)
    P252_WSTEP(t.c, 8, 2 * NL, K)
    E29 r;
    if (WIDE) {
#pragma unroll
        for (int k = 0; k < NL - 1; ++k) {
            P252_TRK_COL(t.c[NL + k]);
            r.d[k] = opaque_digit((int32_t)((uint32_t)t.c[NL + k] ^ 0x80000000u));
            const int64_t h = (int32_t)(t.c[NL + k] >> 32);
            t.c[NL + k + 1] += h * (int64_t)K.eight;
        }
        P252_TRK_COL(t.c[2 * NL - 1]);
        r.d[NL - 1] = opaque_digit((int32_t)t.c[2 * NL - 1]);
        P252_TRK_TOP(r.d[NL - 1]);
        return r;
    }
    int64_t carry = 0;
#pragma unroll
    for (int k = 0; k < NL - 1; ++k) {
        const int64_t v = t.c[NL + k] + carry;
        P252_TRK_COL(t.c[NL + k]);
        r.d[k] = opaque_digit((int32_t)((uint32_t)v & DMASK));
        carry = v >> WB;
    }
    P252_TRK_COL(t.c[2 * NL - 1] + carry);
    r.d[NL - 1] = opaque_digit((int32_t)(t.c[2 * NL - 1] + carry));
    P252_TRK_TOP(r.d[NL - 1]);
    return r;
}

// ---- reduction from the TOP (the integer recurrence of the partial rounds, hades29.hpp::ai_recur) ----
// V = sum c[k] 2^(29 k), nine signed columns, |V| < 2^283 (a sum of nine one-digit multiples of lazy residues).  Instead of
// dividing low digits away (Montgomery steps: 9 multiply-adds per digit, and the value changes scale by 2^-29 each) a
// multiple of p is subtracted that the TOP of the value determines: q = floor(V / 2^252) * M >> 32 with
// M = round(2^284 / p) — the top two columns give V / 2^232 to within 3 units of 2^50, one v_mul_hi_i32 turns that into the
// quotient to within 1.6 — and V - q p is a lazy residue below 1.2 p (|q| < 2^28; simulated over adversarial inputs in
// tests/test_host_arith.py).  Cost: 4 instructions for q, 9 multiply-adds for q p (balanced digits of p, as in the wide
// step), the 8-digit carry chain; the value keeps its scale, so terms of every age enter the recurrence ALIGNED.
#define P252_FOLD_SHIFT 20
#define P252_FOLD_M 592775503 /* round(2^284 / p) */
P252_HD E29 fold_top(int64_t c[NL], const RK& K) {
    P252_TRK_COL(c[NL - 1]);
    const int64_t t = c[NL - 1] + (c[NL - 2] >> WB);
    const int32_t th = opaque_digit((int32_t)(t >> P252_FOLD_SHIFT));
    const int64_t q = opaque_digit((int32_t)(((int64_t)th * (int64_t)P252_FOLD_M) >> 32));
    c[0] += q * (int64_t)K.neg1;
    c[1] += q * (int64_t)K.eight; /* p'_1 = -8 */
    c[2] -= q * (int64_t)P252_PB_2;
    c[3] -= q * (int64_t)P252_PB_3;
    c[4] -= q * (int64_t)P252_PB_4;
    c[5] -= q * (int64_t)P252_PB_5;
    c[6] -= q * (int64_t)P252_PB_6;
    c[7] -= q * (int64_t)P252_PB_7;
    c[8] -= q * (int64_t)P252_PB_8;
    E29 r;
    int64_t carry = 0;
#pragma unroll
    for (int k = 0; k < NL - 1; ++k) {
        const int64_t v = c[k] + carry;
        P252_TRK_COL(c[k]);
        r.d[k] = opaque_digit((int32_t)((uint32_t)v & DMASK));
        carry = v >> WB;
    }
    P252_TRK_COL(c[NL - 1] + carry);
    r.d[NL - 1] = opaque_digit((int32_t)(c[NL - 1] + carry));
    P252_TRK_TOP(r.d[NL - 1]);
    return r;
}

// ---- single-digit linear combinations (the integer MDS layer, hades29.hpp) ----
// R29 holds sum_j n_j * X_j + kappa as nine 64-bit columns (n_j one digit, < 2^18 here).  row_redc1 does
// ONE Montgomery digit step (subtract lo * p, drop the now-zero column) and the carry chain:
// returns (T - lo p) / 2^29 in (T/2^29 - p, T/2^29].  8 + 9 per term instead of 72 + 81 per term.
struct R29 {
    int64_t c[NL];
};
template <class CP>
P252_HD void row_set_c(R29& t, CP kappa) {
#pragma unroll
    for (int k = 0; k < NL; ++k) t.c[k] = kappa[k];
}
P252_HD void row_mac(R29& t, const E29& x, int32_t n) {
    const int64_t nn = n;
#pragma unroll
    for (int k = 0; k < NL; ++k) t.c[k] += (int64_t)x.d[k] * nn;
}
// The value 1 in a form the optimiser cannot see through: (int64)carry * one + column is then ONE
// v_mad_i64_i32 (4 cycles) instead of a sign extension plus a 64-bit add (2 + 4), and the carry itself
// is a v_alignbit_b32 (2 cycles) instead of a 64-bit shift (4).  Row columns stay below 2^59, so their
// carries fit 32 bits (the full redc's columns reach 2^62.5: it keeps 64-bit carries).
P252_HD int32_t opaque_one() {
    int32_t one = 1;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(one));
#endif
    return one;
}
#define P252_ROW_STEP(k, PK)                                                                  \
    {                                                                                         \
        const int64_t v = t.c[k] - lo * (int64_t)(PK) + (int64_t)carry * one;                 \
        r.d[(k) - 1] = opaque_digit((int32_t)((uint32_t)v & DMASK));                          \
        carry = (int32_t)(v >> WB);                                                           \
    }
P252_HD E29 row_redc1(R29& t) {
    const int64_t one = opaque_one();
    const int64_t lo = opaque_digit((int32_t)((uint32_t)t.c[0] & DMASK));
    int32_t carry = (int32_t)(t.c[0] >> WB);
    E29 r;
    P252_ROW_STEP(1, P252_P29_1)
    P252_ROW_STEP(2, P252_P29_2)
    P252_ROW_STEP(3, P252_P29_3)
    P252_ROW_STEP(4, P252_P29_4)
    P252_ROW_STEP(5, P252_P29_5)
    P252_ROW_STEP(6, P252_P29_6)
    P252_ROW_STEP(7, P252_P29_7)
    P252_ROW_STEP(8, P252_P29_8)
    r.d[NL - 1] = opaque_digit(carry);
    return r;
}
#undef P252_ROW_STEP

// Same value, digits NOT carried through: d_k = (column_k mod 2^29) + floor(column_{k-1} / 2^29), so
// |d_k| < 2^30.1 instead of [0, 2^29).  Good enough for a lane that only feeds the next integer layer
// (products with one-digit integers: |column| < 2^18.1 * 2^30.1 + 2^58, carries stay < 2^29.4 — a fixed
// point, not a drift); such a lane must be normalize()d before it enters an S-box.  6 cycles per digit, no chain.
P252_HD E29 row_redc1_lazy(R29& t) {
    const int64_t lo = opaque_digit((int32_t)((uint32_t)t.c[0] & DMASK));
    t.c[1] -= lo * (int64_t)P252_P29_1;
    t.c[2] -= lo * (int64_t)P252_P29_2;
    t.c[3] -= lo * (int64_t)P252_P29_3;
    t.c[4] -= lo * (int64_t)P252_P29_4;
    t.c[5] -= lo * (int64_t)P252_P29_5;
    t.c[6] -= lo * (int64_t)P252_P29_6;
    t.c[7] -= lo * (int64_t)P252_P29_7;
    t.c[8] -= lo * (int64_t)P252_P29_8;
    E29 r;
#pragma unroll
    for (int k = 0; k < NL - 1; ++k)
        r.d[k] = opaque_digit((int32_t)((uint32_t)t.c[1 + k] & DMASK) + (int32_t)(t.c[k] >> WB));
    r.d[NL - 1] = opaque_digit((int32_t)(t.c[NL - 1] >> WB));
    return r;
}

// x * n / R' for a 9-digit constant n (one generic Montgomery product)
template <class CP>
P252_HD E29 mul_c(const E29& x, CP n) {
    A29 t;
    acc_zero(t);
    acc_mul(t, x, n);
    return redc(t);
}

// the same with the wide reduction (result within +-4.01 p of x n / R'); x may have wide digits (n: balanced constant
// digits); WIDE_OUT: the result leaves as wide digits (redc_w)
template <bool WIDE_OUT = false, class CP>
P252_HD E29 mul_c_w(const E29& x, CP n, const RK& K) {
    A29 t;
    acc_zero_w<WIDE_OUT>(t, K);
    acc_mul(t, x, n);
    return redc_w<WIDE_OUT>(t, K);
}

// carry-normalise an element whose digits have drifted (after digit-wise additions)
P252_HD void normalize(E29& x) {
    int32_t carry = 0;
#pragma unroll
    for (int k = 0; k < NL - 1; ++k) {
        const int32_t v = x.d[k] + carry;
        x.d[k] = opaque_digit((int32_t)((uint32_t)v & DMASK));
        carry = v >> WB;
    }
    x.d[NL - 1] += carry;
}

// x += c (digit-wise; c readable as c[k]); result normalised
template <class CP>
P252_HD void add_c(E29& x, CP c) {
#pragma unroll
    for (int k = 0; k < NL; ++k) x.d[k] += c[k];
    normalize(x);
}
P252_HD void add_e(E29& x, const E29& y) { add_c(x, y.d); }

// x -= y (scalar.rs:67-74, Encryption::subtract); signs are tolerated, result normalised
P252_HD void sub_e(E29& x, const E29& y) {
#pragma unroll
    for (int k = 0; k < NL; ++k) x.d[k] -= y.d[k];
    normalize(x);
}

P252_HD E29 e29_zero() {
    E29 r;
#pragma unroll
    for (int k = 0; k < NL; ++k) r.d[k] = 0;
    return r;
}

// x^5 = (x^2)^2 * x  — scalar.rs:50-52.  Three Montgomery products: the result is V^5 / R'^4; the tables
// compensate (sparse schedule: every constant that multiplies an S-box output carries 2^20; integer schedules:
// the factor rides in the scale of the stored state).
P252_HD E29 sbox(const E29& x) {
    A29 t;
    acc_zero(t);
    acc_sqr(t, x);
    const E29 x2 = redc(t);
    acc_zero(t);
    acc_sqr(t, x2);
    const E29 x4 = redc(t);
    acc_zero(t);
    acc_mul(t, x4, x.d);
    return redc(t);
}

// x^5 with wide reductions: |result| < 0.0142 (|x|/p)^2 ... all three stay below 4.4 p for |x| < 7p.  WIDE_OUT: the result
// leaves as wide digits (redc_w) — for outputs that only meet constants (every S-box of the kernels' schedule)
template <bool WIDE_OUT = false>
P252_HD E29 sbox_w(const E29& x, const RK& K) {
    A29 t;
    acc_zero_w(t, K);
    acc_sqr(t, x);
    const E29 x2 = redc_w(t, K);
    acc_zero_w(t, K);
    acc_sqr(t, x2);
    const E29 x4 = redc_w(t, K);
    acc_zero_w<WIDE_OUT>(t, K);
    acc_mul(t, x4, x.d);
    return redc_w<WIDE_OUT>(t, K);
}

// ---- conversion from / to the reference's memory format (4 x u64 Montgomery limbs, R = 2^256) ----
// w[0..7]: the same 32 bytes viewed as 8 little-endian u32 words.
P252_HD E29 from_mont4(const uint32_t w[8]) {
    E29 r;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int bit = WB * i;
        const int q = bit >> 5, s = bit & 31;
        uint64_t window = (uint64_t)w[q];
        if (q + 1 < 8) window |= (uint64_t)w[q + 1] << 32;
        r.d[i] = (int32_t)((uint32_t)(window >> s) & DMASK);
    }
    return r;
}

// Canonicalise: any lazy residue with -2p < V < 3p  ->  the unique limbs in [0, p), as the
// reference's BlsScalar holds them (bit-exact comparison happens on these).  NSUB = conditional subtractions of p:
// 0 < V + 2p < (NSUB + 1) p must hold — 5 in general; the streaming format conversions, whose input is a tight
// reduction of a value below p (-p < V < p), ask for 2.
template <int NSUB = 5>
P252_HD void to_mont4(const E29& x, uint32_t w[8]) {
    // V + 2p > 0, then pack the non-negative value into 9 u32 words
    E29 y = x;
    const int32_t P2[NL] = {2 * P252_P29_0, 2 * P252_P29_1, 2 * P252_P29_2, 2 * P252_P29_3, 2 * P252_P29_4,
                            2 * P252_P29_5, 2 * P252_P29_6, 2 * P252_P29_7, 2 * P252_P29_8};
    {
        int64_t carry = 0;
#pragma unroll
        for (int k = 0; k < NL - 1; ++k) {
            const int64_t v = (int64_t)y.d[k] + P2[k] + carry;
            y.d[k] = (int32_t)((uint32_t)v & DMASK);
            carry = v >> WB;
        }
        y.d[NL - 1] = (int32_t)((int64_t)y.d[NL - 1] + P2[NL - 1] + carry);
    }
    uint32_t u[9];
    {
        // pack 9 x 29 bits into 32-bit words (value < 6p < 2^258 fits 9 words)
        uint64_t acc = 0;
        int bits = 0, k = 0;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            acc |= (uint64_t)(uint32_t)y.d[i] << bits;
            bits += WB;
            if (bits >= 32) {
                u[k++] = (uint32_t)acc;
                acc >>= 32;
                bits -= 32;
            }
        }
        u[k++] = (uint32_t)acc;  // k == 9 here (261 bits -> 8 full words + remainder)
    }
    const uint32_t PW[9] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u,
                            0x3339d808u, 0x299d7d48u, 0x73eda753u, 0u};
    // subtract p while >= p: 0 < V + 2p < 6p  ->  at most 5 conditional subtractions
#pragma unroll
    for (int rep = 0; rep < NSUB; ++rep) {
        uint32_t dif[9];
        uint32_t borrow = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const uint64_t dd = (uint64_t)u[k] - PW[k] - borrow;
            dif[k] = (uint32_t)dd;
            borrow = (uint32_t)(dd >> 63);
        }
        const bool ge = borrow == 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) u[k] = ge ? dif[k] : u[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = u[k];
}

#if defined(__HIPCC__)
// ---- device scalar I/O: one BlsScalar record as it lies in HBM, read and written as two 16-byte accesses ----
struct alignas(16) Scalar32 {
    uint32_t w[8];
};

__device__ __forceinline__ E29 load_scalar(const Scalar32* __restrict__ p) {
    const uint4 lo = *reinterpret_cast<const uint4*>(p);
    const uint4 hi = *(reinterpret_cast<const uint4*>(p) + 1);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return from_mont4(w);
}

__device__ __forceinline__ void store_zero(Scalar32* __restrict__ p) {
    *reinterpret_cast<uint4*>(p) = make_uint4(0u, 0u, 0u, 0u);
    *(reinterpret_cast<uint4*>(p) + 1) = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ void store_scalar(Scalar32* __restrict__ p, const E29& e) {
    uint32_t w[8];
    to_mont4(e, w);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    *(reinterpret_cast<uint4*>(p) + 1) = make_uint4(w[4], w[5], w[6], w[7]);
}

// Hash::finalize_truncated's output (hash.rs:164-183) from the kernel that already holds the value: the canonical
// value (Montgomery form dropped: redc(V * 2^5) = V * 2^5 / 2^261 = V / 2^256) & (2^250 - 1), stored as the raw limbs
// JubJubScalar::from_raw receives.  e is a tight residue (|V| < 2p < 2^256), so the reduction lands in [-p, 0]: two conditional
// subtractions canonicalise.  One product + one reduction per OUTPUT scalar (~110 of a digest's 77,000 instructions) instead of
// a second launch and a 64 B / scalar round trip through HBM (k_to_canonical<true>, kept for scalars that are already stored).
__device__ __forceinline__ void store_truncated(Scalar32* __restrict__ p, const E29& e) {
    const int32_t c32[NL] = {32, 0, 0, 0, 0, 0, 0, 0, 0};
    A29 t;
    acc_zero(t);
    acc_mul(t, e, c32);
    uint32_t w[8];
    to_mont4<2>(redc(t), w);
    w[7] &= 0x03ffffffu;  // TRUNCATION_MASK: keep the low 250 bits
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    *(reinterpret_cast<uint4*>(p) + 1) = make_uint4(w[4], w[5], w[6], w[7]);
}
template <bool TRUNC>
__device__ __forceinline__ void store_output(Scalar32* __restrict__ p, const E29& e) {
    if (TRUNC)
        store_truncated(p, e);
    else
        store_scalar(p, e);
}
#endif  // __HIPCC__

}  // namespace p252
