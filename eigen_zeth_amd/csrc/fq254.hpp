// BN254 base field F_q and the curve code of the multi-scalar multiplication (csrc/msm.hip): F_q and F_q2 in Montgomery form on nine 29-bit
// limbs, the lazy (unreduced) forms of the G1 bucket sums, the Jacobian formulas over both fields, the packed affine point and the signed
// window digits.  Everything is file-local (anonymous namespace): msm.hip, fixed_base.hip and synth.hip include it, and so does
// tests/native/fq254_check.hip, which runs every function at the bounds its comment states.
#pragma once
#include <cstring>

#include "gl.hpp"   // u32, u64

namespace {

// ---- F_q in Montgomery form with R = 2^261: NINE 29-BIT LIMBS.
// v_mad_u64_u32 has a carry-out but no carry-in, so a 32-bit-limb multiplier spends two thirds of its instructions
// moving carries around (the first version compiled to ~790 instructions per product, 47 % of them v_mov).  With
// 29-bit limbs a 64-bit column accumulator takes all 18 products of a column (18 * 2^58 < 2^63) without any carry
// handling: one v_mad_u64_u32 per product, one shift per column -- 162 mads + ~110 other instructions.
// Values are always fully reduced (< q) and normalised (limbs < 2^29) between operations, so equality and the
// infinity tests are plain limb comparisons.
#define FQ_B 29
#define FQ_MASK 0x1FFFFFFFu
#define FQ_INV29 0x04866389u   // -q^-1 mod 2^29
struct fq {
    u32 l[9];
};
#define FQ_HD __host__ __device__ __forceinline__

#define FQ_Q0 0x187cfd47u
#define FQ_Q1 0x010460b6u
#define FQ_Q2 0x1c72a34fu
#define FQ_Q3 0x02d522d0u
#define FQ_Q4 0x1585d978u
#define FQ_Q5 0x02db40c0u
#define FQ_Q6 0x00a6e141u
#define FQ_Q7 0x0e5c2634u
#define FQ_Q8 0x0030644eu
// q as 8 x 32-bit words (exponent bits of the host inversion)
static const u32 FQ_Q_H[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                              0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};

FQ_HD u32 fq_q(int i) {
    switch (i) {
        case 0: return FQ_Q0;
        case 1: return FQ_Q1;
        case 2: return FQ_Q2;
        case 3: return FQ_Q3;
        case 4: return FQ_Q4;
        case 5: return FQ_Q5;
        case 6: return FQ_Q6;
        case 7: return FQ_Q7;
        default: return FQ_Q8;
    }
}
FQ_HD fq fq_zero() {
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = 0;
    return r;
}
FQ_HD fq fq_one() {  // R mod q
    const u32 v[9] = {0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = v[i];
    return r;
}
FQ_HD fq fq_r2() {  // R^2 mod q
    const u32 v[9] = {0x059bac10u, 0x0d1503a3u, 0x018016b8u, 0x10ab0ca8u, 0x02632639u, 0x02c0169fu, 0x169bfd53u, 0x11869d4cu, 0x002a11a6u};
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = v[i];
    return r;
}
FQ_HD bool fq_is_zero(const fq &a) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= a.l[i];
    return o == 0;
}
FQ_HD bool fq_eq(const fq &a, const fq &b) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= a.l[i] ^ b.l[i];
    return o == 0;
}
// t: limbs possibly unnormalised (each < 2^31), value < 2q  ->  normalised value mod q.  Branch-free: both
// the carry-propagated t and t - q are formed, the sign of the last borrow selects.
FQ_HD fq fq_norm_sub(const u32 *t) {
    u32 n[9], d[9];
    int cn = 0, cd = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int vn = (int)t[i] + cn;
        n[i] = (u32)vn & FQ_MASK;
        cn = vn >> FQ_B;
        const int vd = (int)t[i] - (int)fq_q(i) + cd;
        d[i] = (u32)vd & FQ_MASK;
        cd = vd >> FQ_B;   // arithmetic shift: -1 on borrow
    }
    const u32 use_d = cd < 0 ? 0u : 0xFFFFFFFFu;   // no final borrow: t >= q
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = (d[i] & use_d) | (n[i] & ~use_d);
    return r;
}
FQ_HD fq fq_add(const fq &a, const fq &b) {
    u32 t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = a.l[i] + b.l[i];
    return fq_norm_sub(t);
}
FQ_HD fq fq_sub(const fq &a, const fq &b) {
    // a - b, plus q when negative: both chains, select by the final borrow of a - b
    u32 d[9], e[9];
    int cd = 0, ce = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int vd = (int)a.l[i] - (int)b.l[i] + cd;
        d[i] = (u32)vd & FQ_MASK;
        cd = vd >> FQ_B;
        const int ve = (int)a.l[i] - (int)b.l[i] + (int)fq_q(i) + ce;
        e[i] = (u32)ve & FQ_MASK;
        ce = ve >> FQ_B;
    }
    const u32 use_e = cd < 0 ? 0xFFFFFFFFu : 0u;
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = (e[i] & use_e) | (d[i] & ~use_e);
    return r;
}
FQ_HD fq fq_dbl(const fq &a) { return fq_add(a, a); }
// Montgomery product a*b/R mod q, R = 2^261: product scanning, one 64-bit accumulator per column
FQ_HD fq fq_mul(const fq &a, const fq &b) {
    u32 m[9], t[9];
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (u64)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (u64)m[i] * fq_q(k - i);
        m[k] = ((u32)acc * FQ_INV29) & FQ_MASK;
        acc += (u64)m[k] * FQ_Q0;
        acc >>= FQ_B;
    }
#pragma unroll
    for (int k = 9; k < 17; k++) {
#pragma unroll
        for (int i = k - 8; i < 9; i++) {
            acc += (u64)a.l[i] * b.l[k - i];
            acc += (u64)m[i] * fq_q(k - i);
        }
        t[k - 9] = (u32)acc & FQ_MASK;
        acc >>= FQ_B;
    }
    t[8] = (u32)acc;
    return fq_norm_sub(t);   // (ab + mq)/R < q (q/R + 1) < 2q
}
FQ_HD fq fq_sqr(const fq &a) { return fq_mul(a, a); }
FQ_HD fq fq_to_mont(const fq &a) { return fq_mul(a, fq_r2()); }
FQ_HD fq fq_from_mont(const fq &a) {
    fq one = fq_zero();
    one.l[0] = 1;
    return fq_mul(a, one);
}
// 8 x 32-bit words (little endian, value < 2^256... here always < q) <-> 9 x 29-bit limbs
FQ_HD fq fq_from_words(const u32 *w) {
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int bit = FQ_B * i, k = bit >> 5, off = bit & 31;
        u64 v = w[k];
        if (k + 1 < 8) v |= (u64)w[k + 1] << 32;
        r.l[i] = (u32)(v >> off) & FQ_MASK;
    }
    return r;
}
FQ_HD void fq_to_words(const fq &a, u32 *w) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        // word k holds bits [32k, 32k+32): limbs i with 29i < 32k+32 and 29i+29 > 32k
        u64 v = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int lo = FQ_B * i - 32 * k;   // position of limb i relative to word k
            if (lo > -FQ_B && lo < 32) v |= lo >= 0 ? ((u64)a.l[i] << lo) : ((u64)a.l[i] >> (-lo));
        }
        w[k] = (u32)v;
    }
}

// ---- F_q2 = F_q[u]/(u^2 + 1)  (G2 coordinates)
struct fq2 {
    fq c0, c1;
};
FQ_HD fq2 fq2_make(const fq &a, const fq &b) {
    fq2 r;
    r.c0 = a;
    r.c1 = b;
    return r;
}

// ---- lazy (unreduced) arithmetic for the G1 bucket sums.  A point addition is eleven products with a dozen additions and
// subtractions between them; in the canonical form above every one of those normalises and conditionally subtracts q (two
// carry chains and a select, ~90 instructions -- half the instructions of a point addition).  R = 2^261 is 169 q, so a
// Montgomery product only needs  a b < 169 q^2  to return a value < 2 q, and the 64-bit column accumulators take limbs up to
// 2^30.  Between the products values therefore stay congruent but unreduced:
//   N(k): limbs 0..7 < 2^29, value < k q (what lz_mul, lz_sub, lz_carry return);   W(k): limbs < 2^30 (lz_add / lz_dbl of N values)
//   lz_sub<K>(a, b) = a - b + K q with ONE signed carry pass (K q >= b keeps it non-negative): ~45 two-cycle instructions.
// The bounds of every step of the mixed addition are in jac_madd_lazy; results are made canonical once, when a bucket is stored.
constexpr u32 FQ_QL[9] = {FQ_Q0, FQ_Q1, FQ_Q2, FQ_Q3, FQ_Q4, FQ_Q5, FQ_Q6, FQ_Q7, FQ_Q8};
constexpr u32 fq_kq_limb(int K, int i) {            // limb i of K q (normalised limbs, the top one takes the rest)
    u64 carry = 0, v = 0;
    for (int j = 0; j <= i; j++) {
        v = (u64)FQ_QL[j] * (u64)K + carry;
        carry = v >> FQ_B;
    }
    return i == 8 ? (u32)v : (u32)v & FQ_MASK;
}
__device__ __forceinline__ fq lz_mul(const fq &a, const fq &b) {      // limbs < 2^30, a b < 169 q^2  ->  N(1 + a b / 169 q^2)
    u32 m[9];
    fq r;
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (u64)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = 0; i < k; i++) acc += (u64)m[i] * fq_q(k - i);
        m[k] = ((u32)acc * FQ_INV29) & FQ_MASK;
        acc += (u64)m[k] * FQ_Q0;
        acc >>= FQ_B;
    }
#pragma unroll
    for (int k = 9; k < 17; k++) {
#pragma unroll
        for (int i = k - 8; i < 9; i++) {
            acc += (u64)a.l[i] * b.l[k - i];
            acc += (u64)m[i] * fq_q(k - i);
        }
        r.l[k - 9] = (u32)acc & FQ_MASK;
        acc >>= FQ_B;
    }
    r.l[8] = (u32)acc;
    return r;
}
__device__ __forceinline__ fq lz_add(const fq &a, const fq &b) {      // N + N -> W
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
__device__ __forceinline__ fq lz_dbl(const fq &a) {                   // N -> W
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] << 1;
    return r;
}
__device__ __forceinline__ fq lz_quad(const fq &a) {                  // 4 a, carried: N -> N
    fq r;
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const u32 v = (a.l[i] << 2) + c;
        r.l[i] = i < 8 ? (v & FQ_MASK) : v;
        c = v >> FQ_B;
    }
    return r;
}
template <int K>
__device__ __forceinline__ fq lz_sub(const fq &a, const fq &b) {      // a - b + K q  (K q >= b):  -> N(a + K)
    fq r;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int v = (int)a.l[i] - (int)b.l[i] + (int)fq_kq_limb(K, i) + c;
        r.l[i] = i < 8 ? ((u32)v & FQ_MASK) : (u32)v;
        c = v >> FQ_B;        // arithmetic shift: floor division
    }
    return r;
}
template <int K>
__device__ __forceinline__ fq lz_sub2(const fq &a, const fq &b, const fq &d) {   // a - b - d + K q  (K q >= b + d)
    fq r;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int v = (int)a.l[i] - (int)b.l[i] - (int)d.l[i] + (int)fq_kq_limb(K, i) + c;
        r.l[i] = i < 8 ? ((u32)v & FQ_MASK) : (u32)v;
        c = v >> FQ_B;
    }
    return r;
}
__device__ __forceinline__ bool lz_is_zero_mod_q(const fq &a) {       // a in N(2): congruent to 0 iff a is 0 or q
    u32 z = 0, e = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) { z |= a.l[i]; e |= a.l[i] ^ FQ_QL[i]; }
    return z == 0 || e == 0;
}
__device__ __forceinline__ fq lz_canon(const fq &a) { return fq_mul(a, fq_one()); }   // a R / R mod q, fully reduced (limbs < 2^30, a < 169 q)

// ---- one set of names over both fields, so that the curve code and the kernels are written once
template <class F> struct FT;
template <> struct FT<fq> {
    static constexpr int WORDS = 8;   // 32-bit words of one packed element
    static FQ_HD fq zero() { return fq_zero(); }
    static FQ_HD fq one() { return fq_one(); }
    static FQ_HD fq from_words(const u32 *w) { return fq_from_words(w); }
    static FQ_HD void to_words(const fq &a, u32 *w) { fq_to_words(a, w); }
};
template <> struct FT<fq2> {
    static constexpr int WORDS = 16;
    static FQ_HD fq2 zero() { return fq2_make(fq_zero(), fq_zero()); }
    static FQ_HD fq2 one() { return fq2_make(fq_one(), fq_zero()); }
    static FQ_HD fq2 from_words(const u32 *w) { return fq2_make(fq_from_words(w), fq_from_words(w + 8)); }
    static FQ_HD void to_words(const fq2 &a, u32 *w) {
        fq_to_words(a.c0, w);
        fq_to_words(a.c1, w + 8);
    }
};
FQ_HD bool f_is_zero(const fq &a) { return fq_is_zero(a); }
FQ_HD bool f_eq(const fq &a, const fq &b) { return fq_eq(a, b); }
FQ_HD fq f_add(const fq &a, const fq &b) { return fq_add(a, b); }
FQ_HD fq f_sub(const fq &a, const fq &b) { return fq_sub(a, b); }
FQ_HD fq f_dbl(const fq &a) { return fq_dbl(a); }
FQ_HD fq f_mul(const fq &a, const fq &b) { return fq_mul(a, b); }
FQ_HD fq f_sqr(const fq &a) { return fq_sqr(a); }
FQ_HD fq f_to_mont(const fq &a) { return fq_to_mont(a); }
FQ_HD fq f_from_mont(const fq &a) { return fq_from_mont(a); }
FQ_HD bool f_is_zero(const fq2 &a) { return fq_is_zero(a.c0) && fq_is_zero(a.c1); }
FQ_HD bool f_eq(const fq2 &a, const fq2 &b) { return fq_eq(a.c0, b.c0) && fq_eq(a.c1, b.c1); }
FQ_HD fq2 f_add(const fq2 &a, const fq2 &b) { return fq2_make(fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)); }
FQ_HD fq2 f_sub(const fq2 &a, const fq2 &b) { return fq2_make(fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)); }
FQ_HD fq2 f_dbl(const fq2 &a) { return fq2_make(fq_dbl(a.c0), fq_dbl(a.c1)); }
// (a b + c d) / R mod q with ONE Montgomery reduction: the two products share the column accumulators (27 terms of < 2^58 per
// column stay below 2^64).  Limbs < 2^29 (one operand of each product may have limbs < 2^30), a b + c d < 169 q^2.
FQ_HD fq fq_mul2(const fq &a, const fq &b, const fq &c, const fq &d) {
    u32 m[9], t[9];
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) {
            acc += (u64)a.l[i] * b.l[k - i];
            acc += (u64)c.l[i] * d.l[k - i];
        }
#pragma unroll
        for (int i = 0; i < k; i++) acc += (u64)m[i] * fq_q(k - i);
        m[k] = ((u32)acc * FQ_INV29) & FQ_MASK;
        acc += (u64)m[k] * FQ_Q0;
        acc >>= FQ_B;
    }
#pragma unroll
    for (int k = 9; k < 17; k++) {
#pragma unroll
        for (int i = k - 8; i < 9; i++) {
            acc += (u64)a.l[i] * b.l[k - i];
            acc += (u64)c.l[i] * d.l[k - i];
            acc += (u64)m[i] * fq_q(k - i);
        }
        t[k - 9] = (u32)acc & FQ_MASK;
        acc >>= FQ_B;
    }
    t[8] = (u32)acc;
    return fq_norm_sub(t);   // (ab + cd + mq)/R < q (2q/R + 1) < 2q
}
// q - a in (0, q] with one signed carry pass (a canonical); congruent to -a, limbs < 2^29
FQ_HD fq fq_neg_lazy(const fq &a) {
    fq r;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int v = (int)fq_q(i) - (int)a.l[i] + c;
        r.l[i] = i < 8 ? ((u32)v & FQ_MASK) : (u32)v;
        c = v >> FQ_B;
    }
    return r;
}
// F_q2 products with the reduction delayed over the two terms of each component (no Karatsuba: the same 486 limb products,
// two Montgomery reductions instead of three and none of its five additions / subtractions):
//   (a0 + a1 u)(b0 + b1 u) = (a0 b0 + (q - a1) b1) + (a0 b1 + a1 b0) u
FQ_HD fq2 f_mul(const fq2 &a, const fq2 &b) {
    return fq2_make(fq_mul2(a.c0, b.c0, fq_neg_lazy(a.c1), b.c1), fq_mul2(a.c0, b.c1, a.c1, b.c0));
}
FQ_HD fq2 f_sqr(const fq2 &a) {   // (a0 a0 + (q - a1) a1) + (a0 * 2 a1) u
    fq d;
#pragma unroll
    for (int i = 0; i < 9; i++) d.l[i] = a.c1.l[i] << 1;      // 2 a1, limbs < 2^30
    return fq2_make(fq_mul2(a.c0, a.c0, fq_neg_lazy(a.c1), a.c1), fq_mul(a.c0, d));
}
FQ_HD fq2 f_to_mont(const fq2 &a) { return fq2_make(fq_to_mont(a.c0), fq_to_mont(a.c1)); }
FQ_HD fq2 f_from_mont(const fq2 &a) { return fq2_make(fq_from_mont(a.c0), fq_from_mont(a.c1)); }

// ---- short Weierstrass curve y^2 = x^3 + b (a = 0) in Jacobian coordinates over F (G1: F_q, G2: F_q2)
template <class F>
struct jacT {
    F X, Y, Z;  // Z == 0: point at infinity
};
template <class F>
FQ_HD jacT<F> jac_inf() {
    jacT<F> p;
    p.X = FT<F>::one();
    p.Y = FT<F>::one();
    p.Z = FT<F>::zero();
    return p;
}
// dbl-2009-l (a = 0)
template <class F>
FQ_HD jacT<F> jac_dbl(const jacT<F> &p) {
    if (f_is_zero(p.Z)) return p;
    F A = f_sqr(p.X), B = f_sqr(p.Y), C = f_sqr(B);
    F t = f_add(p.X, B);
    F D = f_dbl(f_sub(f_sub(f_sqr(t), A), C));
    F E = f_add(f_dbl(A), A);
    F G = f_sqr(E);
    jacT<F> r;
    r.X = f_sub(G, f_dbl(D));
    F C8 = f_dbl(f_dbl(f_dbl(C)));
    r.Y = f_sub(f_mul(E, f_sub(D, r.X)), C8);
    r.Z = f_dbl(f_mul(p.Y, p.Z));
    return r;
}
// madd-2007-bl: Jacobian + affine (qx, qy) (affine point must not be infinity)
template <class F>
FQ_HD jacT<F> jac_madd(const jacT<F> &p, const F &qx, const F &qy) {
    if (f_is_zero(p.Z)) {
        jacT<F> r;
        r.X = qx;
        r.Y = qy;
        r.Z = FT<F>::one();
        return r;
    }
    F Z1Z1 = f_sqr(p.Z);
    F U2 = f_mul(qx, Z1Z1);
    F S2 = f_mul(f_mul(qy, p.Z), Z1Z1);
    if (f_eq(U2, p.X)) {
        if (f_eq(S2, p.Y)) return jac_dbl(p);
        return jac_inf<F>();
    }
    F H = f_sub(U2, p.X);
    F HH = f_sqr(H);
    F I = f_dbl(f_dbl(HH));
    F J = f_mul(H, I);
    F rr = f_dbl(f_sub(S2, p.Y));
    F V = f_mul(p.X, I);
    jacT<F> r;
    r.X = f_sub(f_sub(f_sqr(rr), J), f_dbl(V));
    r.Y = f_sub(f_mul(rr, f_sub(V, r.X)), f_dbl(f_mul(p.Y, J)));
    r.Z = f_sub(f_sub(f_sqr(f_add(p.Z, H)), Z1Z1), HH);
    return r;
}
// madd-2007-bl on lazy values (G1 bucket sums).  Invariant of the accumulator between calls (units of q):
//   X in N(7), Y in N(5), Z in W(2.3);  the affine point is canonical.  Bounds of every step, with lz_mul -> 1 + a b / 169:
//   Z1Z1, U2, t, S2 < 2;  H = U2 - X + 7q < 8.02;  HH < 1.38;  I = 4 HH < 5.52;  J = H I -> < 1.27;  V = X I -> < 1.23;
//   r0 = S2 - Y + 5q < 6.02, rr = 2 r0 < 12.03 (W), rr^2 -> < 1.86;  X3 = rr^2 - J - 2V + 4q < 5.86  (J + 2V < 3.73);
//   V - X3 + 6q < 7.23, rr (V - X3) -> < 1.52;  Y J -> < 1.04;  Y3 = .. - 2 Y J + 3q < 4.52;  Z3 = 2 (Z H) < 2.22 (W).
// H == 0 mod q (the point equals +-the accumulator: doubling or infinity) is detected on HH, which lz_mul returns in
// N(2) with exact limbs, and handled by the canonical code on canonicalised inputs.
__device__ __forceinline__ jacT<fq> jac_madd_lazy(const jacT<fq> &p, const fq &qx, const fq &qy) {
    if (fq_is_zero(p.Z)) {            // infinity is always the exact zero
        jacT<fq> r;
        r.X = qx;
        r.Y = qy;
        r.Z = fq_one();
        return r;
    }
    const fq Z1Z1 = lz_mul(p.Z, p.Z);
    const fq U2 = lz_mul(qx, Z1Z1);
    const fq S2 = lz_mul(lz_mul(qy, p.Z), Z1Z1);
    const fq H = lz_sub<7>(U2, p.X);
    const fq HH = lz_mul(H, H);
    if (lz_is_zero_mod_q(HH)) {
        jacT<fq> c;
        c.X = lz_canon(p.X);
        c.Y = lz_canon(p.Y);
        c.Z = lz_canon(p.Z);
        return jac_madd(c, qx, qy);   // canonical: doubles or returns the exact infinity
    }
    const fq I = lz_quad(HH);
    const fq J = lz_mul(H, I);
    const fq rr = lz_dbl(lz_sub<5>(S2, p.Y));
    const fq V = lz_mul(p.X, I);
    jacT<fq> r;
    r.X = lz_sub2<4>(lz_mul(rr, rr), J, lz_dbl(V));
    r.Y = lz_sub<3>(lz_mul(rr, lz_sub<6>(V, r.X)), lz_dbl(lz_mul(p.Y, J)));
    r.Z = lz_dbl(lz_mul(p.Z, H));
    return r;
}
__device__ __forceinline__ jacT<fq> jac_canon(const jacT<fq> &p) {
    jacT<fq> r;
    r.X = lz_canon(p.X);
    r.Y = lz_canon(p.Y);
    r.Z = lz_canon(p.Z);
    return r;
}
__device__ __forceinline__ jacT<fq2> jac_canon(const jacT<fq2> &p) { return p; }   // G2 sums stay canonical throughout

// add-2007-bl: Jacobian + Jacobian
template <class F>
FQ_HD jacT<F> jac_add(const jacT<F> &p, const jacT<F> &q) {
    if (f_is_zero(p.Z)) return q;
    if (f_is_zero(q.Z)) return p;
    F Z1Z1 = f_sqr(p.Z), Z2Z2 = f_sqr(q.Z);
    F U1 = f_mul(p.X, Z2Z2), U2 = f_mul(q.X, Z1Z1);
    F S1 = f_mul(f_mul(p.Y, q.Z), Z2Z2), S2 = f_mul(f_mul(q.Y, p.Z), Z1Z1);
    if (f_eq(U1, U2)) {
        if (f_eq(S1, S2)) return jac_dbl(p);
        return jac_inf<F>();
    }
    F H = f_sub(U2, U1);
    F I = f_sqr(f_dbl(H));
    F J = f_mul(H, I);
    F rr = f_dbl(f_sub(S2, S1));
    F V = f_mul(U1, I);
    jacT<F> r;
    r.X = f_sub(f_sub(f_sqr(rr), J), f_dbl(V));
    r.Y = f_sub(f_mul(rr, f_sub(V, r.X)), f_dbl(f_mul(S1, J)));
    r.Z = f_mul(f_sub(f_sub(f_sqr(f_add(p.Z, q.Z)), Z1Z1), Z2Z2), H);
    return r;
}
template <class F>
FQ_HD jacT<F> jac_mul_small(const jacT<F> &p, u32 k) {  // k * p by double-and-add (k < 2^32)
    jacT<F> acc = jac_inf<F>();
    int top = 31;
    while (top > 0 && !((k >> top) & 1)) top--;   // skip the leading zero bits (doublings of the point at infinity)
    for (int i = top; i >= 0; i--) {
        acc = jac_dbl(acc);
        if ((k >> i) & 1) acc = jac_add(acc, p);
    }
    return acc;
}

// a packed affine point = 2 * FT<F>::WORDS words = NV uint4 (G1: 4, G2: 8); (0, 0) encodes the point at infinity
#if defined(__HIPCC__)   // (uint4: the host-only build of tests/native/fq254_check.hip has no such type)
template <class F>
__device__ __forceinline__ void unpack_point(const uint4 *q, F &x, F &y) {
    constexpr int NV = FT<F>::WORDS / 2;
    u32 w[FT<F>::WORDS * 2];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        w[4 * k] = q[k].x;
        w[4 * k + 1] = q[k].y;
        w[4 * k + 2] = q[k].z;
        w[4 * k + 3] = q[k].w;
    }
    x = FT<F>::from_words(w);
    y = FT<F>::from_words(w + FT<F>::WORDS);
}
#endif

// Signed window digits.  With K = sum_w 2^(cd w + cd - 1) the unsigned digits u_w of s + K give  s = sum_w (u_w - 2^(cd-1)) 2^(cd w):
// digits d_w in [-2^(cd-1), 2^(cd-1)), so a window has 2^(cd-1) buckets |d| = 1 .. 2^(cd-1) (bucket index |d| - 1) and a negative
// digit adds -P.  One more bit of window for the same bucket memory: 14 windows of 19 bits instead of 15 of 18.
// sc9 = s + K as nine 32-bit words (carry-propagated once per scalar); returns |d| (0: skip) and the sign.
__device__ __forceinline__ void add_bias9(const u32 *sc, const u32 *K, u32 *s9) {
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        c += (u64)(j < 8 ? sc[j] : 0u) + K[j];
        s9[j] = (u32)c;
        c >>= 32;
    }
}
__device__ __forceinline__ u32 digit_key(const u32 *s9, int w, int cd, u32 &neg) {
    const int bit = w * cd;
    const int limb = bit >> 5, off = bit & 31;
    u64 v = s9[limb];
    if (limb + 1 < 9) v |= (u64)s9[limb + 1] << 32;
    const int d = (int)((u32)(v >> off) & ((1u << cd) - 1)) - (1 << (cd - 1));
    neg = d < 0 ? 1u : 0u;
    return (u32)(d < 0 ? -d : d);
}

fq fq_inv_host(const fq &a) {  // a^(q-2) in Montgomery form (host, once per MSM)
    u32 e[8];
    memcpy(e, FQ_Q_H, sizeof(e));
    e[0] -= 2;  // q is odd and its low limb is > 2
    fq r = fq_one(), b = a;
    for (int i = 0; i < 256; i++) {
        if ((e[i >> 5] >> (i & 31)) & 1) r = fq_mul(r, b);
        b = fq_sqr(b);
    }
    return r;
}
fq f_inv_host(const fq &a) { return fq_inv_host(a); }
fq2 f_inv_host(const fq2 &a) {  // (a0 - a1 u) / (a0^2 + a1^2)
    const fq d = fq_inv_host(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)));
    return fq2_make(fq_mul(a.c0, d), fq_sub(fq_zero(), fq_mul(a.c1, d)));
}
// the affine words (standard form, x then y: the layout of the MSM entry points) of a Jacobian point with Z != 0, given zi = 1 / Z
template <class F>
void jac_affine_words(const jacT<F> &p, const F &zi, u32 *out) {
    const F zi2 = f_sqr(zi);
    FT<F>::to_words(f_from_mont(f_mul(p.X, zi2)), out);
    FT<F>::to_words(f_from_mont(f_mul(p.Y, f_mul(zi2, zi))), out + FT<F>::WORDS);
}

}  // namespace
