// The optimal-ate pairing on BN254 (alt_bn128) for csrc/pairing.hip: the Fermat inverse in F_q and F_q2, the degree-12 extension
// F_q12 = F_q2[w]/(w^6 - xi), xi = 9 + u, the Miller loop over 6x + 2 with the two Frobenius line steps, the final exponentiation to EXACTLY
// (q^12 - 1)/r, and the point checks (on the curve, on the twist y^2 = x^3 + 3/xi, [r]Q = O).  Montgomery limbs (csrc/fq254.hpp) inside,
// standard-form words only at the boundary.  File-local like fq254.hpp; tests/native/pairing254_check.cpp runs every function.
//
// Shape of the code: written in fq254.hpp's host-and-device form (FQ_HD, P12_FN) with fixed trip counts and branches on constants only, so that a
// lane-per-job kernel can run it unchanged -- but only the host runs it today.  The F_q2 product is the unit that inlines;
// everything above it is a P12_FN function (not inlined) whose loops over the tower coefficients stay loops, so that a caller holds one copy of
// each product.  An F_q12 value is six F_q2 coefficients in memory.
//
// GT values leave in the flat basis F_q[w]/(w^12 - 18 w^6 + 82) (u = w^6 - 9): (a_i + b_i u) w^i gives a_i - 9 b_i at w^i and b_i at w^(i+6).
// Lines are scaled by factors in F_q2, which the final exponentiation kills ((q^6 - 1) is a multiple of q^2 - 1): a Miller value is defined up to
// such a factor, a GT value is exact.
#pragma once
#include "fq254.hpp"

#define P12_FN __host__ __device__ __attribute__((noinline))

namespace {

#include "pairing254_constants.inc"

#define P12_ATE_LOW 11347224129447541672ULL   // 6x + 2 = 29793968203157093288 = 2^64 + this: the loop starts at the point itself and walks bits 63 .. 0
#define P12_X 4965661367192848881ULL          // the BN parameter x (63 bits)

FQ_HD fq fq_ld(const u32 *w) {
    fq r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = w[i];
    return r;
}
FQ_HD fq2 fq2_ld(const u32 *w) { return fq2_make(fq_ld(w), fq_ld(w + 9)); }
FQ_HD fq fq_neg(const fq &a) { return fq_sub(fq_zero(), a); }
FQ_HD fq2 fq2_neg(const fq2 &a) { return fq2_make(fq_neg(a.c0), fq_neg(a.c1)); }
FQ_HD fq2 fq2_conj(const fq2 &a) { return fq2_make(a.c0, fq_neg(a.c1)); }
FQ_HD fq2 fq2_scale(const fq2 &a, const fq &s) { return fq2_make(fq_mul(a.c0, s), fq_mul(a.c1, s)); }
FQ_HD fq fq_x9(const fq &a) {
    const fq a8 = fq_dbl(fq_dbl(fq_dbl(a)));
    return fq_add(a8, a);
}
FQ_HD fq2 fq2_mul_xi(const fq2 &a) {   // (a0 + a1 u)(9 + u) = (9 a0 - a1) + (a0 + 9 a1) u
    return fq2_make(fq_sub(fq_x9(a.c0), a.c1), fq_add(a.c0, fq_x9(a.c1)));
}
FQ_HD u32 p12_r_word(int i) {   // the group order r, 32-bit words
    switch (i) {
        case 0: return 0xf0000001u;
        case 1: return 0x43e1f593u;
        case 2: return 0x79b97091u;
        case 3: return 0x2833e848u;
        case 4: return 0x8181585du;
        case 5: return 0xb85045b6u;
        case 6: return 0xe131a029u;
        default: return 0x30644e72u;
    }
}

// a^(q - 2) over the bits of FQ_Q_H (Fermat): the inverse, 0 for 0.  Fixed trip count, the branch is on a bit of q (fq_inv_host's twin, device-callable)
P12_FN fq fq_inv(const fq &a) {
    fq r = fq_one(), b = a;
#pragma unroll 1
    for (int w = 0; w < 8; w++) {
        const u32 e = FQ_Q_H[w] - (w == 0 ? 2u : 0u);   // q is odd and its low word is > 2
#pragma unroll 1
        for (int i = 0; i < 32; i++) {
            if ((e >> i) & 1) r = fq_mul(r, b);
            b = fq_sqr(b);
        }
    }
    return r;
}
P12_FN fq2 fq2_inv(const fq2 &a) {   // (a0 - a1 u) / (a0^2 + a1^2)
    const fq d = fq_inv(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)));
    return fq2_make(fq_mul(a.c0, d), fq_neg(fq_mul(a.c1, d)));
}

// ---- F_q12 = F_q2[w]/(w^6 - xi)
struct fq12 {
    fq2 c[6];
};
P12_FN void fq12_set_one(fq12 &r) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) r.c[i] = FT<fq2>::zero();
    r.c[0] = FT<fq2>::one();
}
P12_FN bool fq12_is_one(const fq12 &a) {
    bool ok = f_eq(a.c[0], FT<fq2>::one());
#pragma unroll 1
    for (int i = 1; i < 6; i++) ok = ok & f_is_zero(a.c[i]);
    return ok;
}
// coefficient k of a product is completed in registers (the terms below w^6 and the ones that wrap, which take one xi) and then stored
P12_FN void fq12_mul(fq12 &r, const fq12 &a, const fq12 &b) {
    fq12 t;
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
        fq2 lo = FT<fq2>::zero(), hi = FT<fq2>::zero();
#pragma unroll 1
        for (int i = 0; i < 6; i++) {
            const int j = k - i;
            const fq2 p = f_mul(a.c[i], b.c[j < 0 ? j + 6 : j]);
            if (j < 0) hi = f_add(hi, p);
            else lo = f_add(lo, p);
        }
        t.c[k] = f_add(lo, fq2_mul_xi(hi));
    }
    r = t;
}
P12_FN void fq12_sqr(fq12 &r, const fq12 &a) { fq12_mul(r, a, a); }
// the sparse product by a line l0 + l1 w + l3 w^3
P12_FN void fq12_mul_line(fq12 &r, const fq12 &a, const fq2 &l0, const fq2 &l1, const fq2 &l3) {
    fq12 t;
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
        fq2 lo = f_mul(a.c[k], l0), hi = FT<fq2>::zero();
        const fq2 p1 = f_mul(a.c[k >= 1 ? k - 1 : k + 5], l1);
        if (k >= 1) lo = f_add(lo, p1);
        else hi = p1;
        const fq2 p3 = f_mul(a.c[k >= 3 ? k - 3 : k + 3], l3);
        if (k >= 3) lo = f_add(lo, p3);
        else hi = f_add(hi, p3);
        t.c[k] = f_add(lo, fq2_mul_xi(hi));
    }
    r = t;
}
// the q^6-power map: w -> -w.  On the cyclotomic subgroup (after the easy part of the final exponentiation) it is the inverse
P12_FN void fq12_conj(fq12 &r, const fq12 &a) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) r.c[i] = (i & 1) ? fq2_neg(a.c[i]) : a.c[i];
}
// the q^k-power map, k = 1, 2, 3: w^i -> xi^(i (q^k - 1) / 6) w^i, coefficients conjugated for odd k
P12_FN void fq12_frob(fq12 &r, const fq12 &a, int k) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const fq2 c = (k & 1) ? fq2_conj(a.c[i]) : a.c[i];
        r.c[i] = f_mul(c, fq2_ld(P12_FROB[k - 1][i]));
    }
}
// 1 / a through norms: N = a conj(a) lies in F_q6, N N^(q^2) N^(q^4) in F_q2, so  1/a = conj(a) N^(q^2) N^(q^4) / (that element).  0 gives 0
P12_FN void fq12_inv(fq12 &r, const fq12 &a) {
    fq12 c, n, n2, m;
    fq12_conj(c, a);
    fq12_mul(n, a, c);
    fq12_frob(n2, n, 2);
    fq12_frob(m, n2, 2);
    fq12_mul(m, m, n2);
    fq12_mul(n, n, m);
    const fq2 d = fq2_inv(n.c[0]);
    fq12_mul(c, c, m);
#pragma unroll 1
    for (int i = 0; i < 6; i++) r.c[i] = f_mul(c.c[i], d);
}
// 96 standard-form words in the flat basis
P12_FN void fq12_to_flat_words(const fq12 &a, u32 *out) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        fq_to_words(fq_from_mont(fq_sub(a.c[i].c0, fq_x9(a.c[i].c1))), out + 8 * i);
        fq_to_words(fq_from_mont(a.c[i].c1), out + 8 * (i + 6));
    }
}
// the tower element of 12 flat coefficients given as Montgomery limbs (the check program's way in): b_i = flat[i + 6], a_i = flat[i] + 9 b_i
P12_FN void fq12_from_flat(fq12 &r, const u32 *limbs) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const fq b = fq_ld(limbs + 9 * (i + 6));
        r.c[i] = fq2_make(fq_add(fq_ld(limbs + 9 * i), fq_x9(b)), b);
    }
}
P12_FN void fq12_to_flat(const fq12 &a, u32 *limbs) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const fq lo = fq_sub(a.c[i].c0, fq_x9(a.c[i].c1));
#pragma unroll
        for (int l = 0; l < 9; l++) {
            limbs[9 * i + l] = lo.l[l];
            limbs[9 * (i + 6) + l] = a.c[i].c1.l[l];
        }
    }
}

// ---- the Miller loop.  T is Jacobian on the twist, Q = (x2, y2) affine, P = (xP, yP) in G1.  With the untwist (x, y) -> (x w^2, y w^3) the line
// through T of slope m on the twist is  -yP + m xP w + (yT - m xT) w^3  at P; each step scales it by an F_q2 factor that clears the denominators.
// doubling (dbl-2009-l): m = 3 X^2 / Z3, Z3 = 2 Y Z; times Z3 Z^2:  l0 = -(Z3 Z^2) yP,  l1 = (3 X^2 Z^2) xP,  l3 = 2 Y^2 - 3 X^3
P12_FN void p12_dbl_step(jacT<fq2> &T, const fq &xP, const fq &nyP, fq2 &l0, fq2 &l1, fq2 &l3) {
    const fq2 A = f_sqr(T.X), B = f_sqr(T.Y), C = f_sqr(B), Z2 = f_sqr(T.Z);
    const fq2 D = f_dbl(f_sub(f_sub(f_sqr(f_add(T.X, B)), A), C));
    const fq2 E = f_add(f_dbl(A), A);
    const fq2 Z3 = f_dbl(f_mul(T.Y, T.Z));
    l0 = fq2_scale(f_mul(Z3, Z2), nyP);
    l1 = fq2_scale(f_mul(E, Z2), xP);
    l3 = f_sub(f_dbl(B), f_mul(E, T.X));
    const fq2 X3 = f_sub(f_sqr(E), f_dbl(D));
    T.Y = f_sub(f_mul(E, f_sub(D, X3)), f_dbl(f_dbl(f_dbl(C))));
    T.X = X3;
    T.Z = Z3;
}
// addition (madd-2007-bl): m = rr / Z3 with rr = 2 (y2 Z^3 - Y), Z3 = 2 Z H; times Z3:  l0 = -Z3 yP,  l1 = rr xP,  l3 = Z3 y2 - rr x2.
// No case split: T = +-Q does not occur for a point of order r (the loop's multiples of Q stay below r)
P12_FN void p12_add_step(jacT<fq2> &T, const fq2 &x2, const fq2 &y2, const fq &xP, const fq &nyP, fq2 &l0, fq2 &l1, fq2 &l3) {
    const fq2 Z1Z1 = f_sqr(T.Z);
    const fq2 H = f_sub(f_mul(x2, Z1Z1), T.X);
    const fq2 rr = f_dbl(f_sub(f_mul(f_mul(y2, T.Z), Z1Z1), T.Y));
    const fq2 HH = f_sqr(H);
    const fq2 I = f_dbl(f_dbl(HH));
    const fq2 J = f_mul(H, I), V = f_mul(T.X, I);
    const fq2 Z3 = f_sub(f_sub(f_sqr(f_add(T.Z, H)), Z1Z1), HH);
    l0 = fq2_scale(Z3, nyP);
    l1 = fq2_scale(rr, xP);
    l3 = f_sub(f_mul(Z3, y2), f_mul(rr, x2));
    const fq2 X3 = f_sub(f_sub(f_sqr(rr), J), f_dbl(V));
    T.Y = f_sub(f_mul(rr, f_sub(V, X3)), f_dbl(f_mul(T.Y, J)));
    T.X = X3;
    T.Z = Z3;
}
// f = the Miller value of (P, Q), both affine, finite and valid (Montgomery form).  64 doubling steps, the additions at the set bits of 6x + 2,
// then Q1 = pi(Q) and -pi^2(Q): the trip count and every branch depend on constants alone
P12_FN void p12_miller(fq12 &f, const fq &xP, const fq &yP, const fq2 &xQ, const fq2 &yQ) {
    const fq nyP = fq_neg(yP);
    jacT<fq2> T;
    T.X = xQ;
    T.Y = yQ;
    T.Z = FT<fq2>::one();
    fq2 l0, l1, l3;
    fq12_set_one(f);
#pragma unroll 1
    for (int i = 63; i >= 0; i--) {
        fq12_sqr(f, f);
        p12_dbl_step(T, xP, nyP, l0, l1, l3);
        fq12_mul_line(f, f, l0, l1, l3);
        if ((P12_ATE_LOW >> i) & 1) {
            p12_add_step(T, xQ, yQ, xP, nyP, l0, l1, l3);
            fq12_mul_line(f, f, l0, l1, l3);
        }
    }
    const fq2 x1 = f_mul(fq2_conj(xQ), fq2_ld(P12_FROB[0][2])), y1 = f_mul(fq2_conj(yQ), fq2_ld(P12_FROB[0][3]));
    p12_add_step(T, x1, y1, xP, nyP, l0, l1, l3);
    fq12_mul_line(f, f, l0, l1, l3);
    const fq2 x2 = f_mul(xQ, fq2_ld(P12_FROB[1][2])), y2 = fq2_neg(f_mul(yQ, fq2_ld(P12_FROB[1][3])));
    p12_add_step(T, x2, y2, xP, nyP, l0, l1, l3);
    fq12_mul_line(f, f, l0, l1, l3);
}

// ---- the final exponentiation
P12_FN void fq12_pow_x(fq12 &r, const fq12 &a) {   // a^x, square and multiply over the 63 bits of x
    fq12 t = a;
#pragma unroll 1
    for (int i = 61; i >= 0; i--) {
        fq12_sqr(t, t);
        if ((P12_X >> i) & 1) fq12_mul(t, t, a);
    }
    r = t;
}
// r = f^((q^12 - 1)/r), exactly.  Easy part: m = f^((q^6 - 1)(q^2 + 1)).  Hard part (Devegili, Scott, Dahab):
//   (q^4 - q^2 + 1)/r = q^3 + (6x^2 + 1) q^2 + (-36x^3 - 18x^2 - 12x + 1) q + (-36x^3 - 30x^2 - 18x - 2)
// as  y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36  with  y0 = m^q m^(q^2) m^(q^3), y1 = 1/m, y2 = (m^(x^2))^(q^2), y3 = 1/(m^x)^q,
// y4 = 1/(m^x (m^(x^2))^q), y5 = 1/m^(x^2), y6 = 1/(m^(x^3) (m^(x^3))^q); inverses are conjugates here.  0 gives 0
P12_FN void fq12_final_exp(fq12 &r, const fq12 &f) {
    fq12 m, t0, t1, a, b, fx, fx2, fx3;
    fq12_inv(t0, f);
    fq12_conj(t1, f);
    fq12_mul(t0, t0, t1);          // f^(q^6 - 1)
    fq12_frob(t1, t0, 2);
    fq12_mul(m, t1, t0);
    fq12_pow_x(fx, m);
    fq12_pow_x(fx2, fx);
    fq12_pow_x(fx3, fx2);
    // t0 = y6^2 y4 y5
    fq12_frob(a, fx3, 1);
    fq12_mul(a, a, fx3);
    fq12_conj(a, a);               // y6
    fq12_sqr(t0, a);
    fq12_frob(a, fx2, 1);
    fq12_mul(a, a, fx);
    fq12_conj(a, a);               // y4
    fq12_mul(t0, t0, a);
    fq12_conj(b, fx2);             // y5
    fq12_mul(t0, t0, b);
    // t1 = y3 y5 t0
    fq12_frob(a, fx, 1);
    fq12_conj(a, a);               // y3
    fq12_mul(t1, a, b);
    fq12_mul(t1, t1, t0);
    fq12_frob(a, fx2, 2);          // y2
    fq12_mul(t0, t0, a);
    fq12_sqr(t1, t1);
    fq12_mul(t1, t1, t0);
    fq12_sqr(t1, t1);
    fq12_conj(a, m);               // y1
    fq12_mul(t0, t1, a);
    fq12_frob(a, m, 1);
    fq12_frob(b, m, 2);
    fq12_mul(a, a, b);
    fq12_frob(b, m, 3);
    fq12_mul(a, a, b);             // y0
    fq12_mul(t1, t1, a);
    fq12_sqr(t0, t0);
    fq12_mul(r, t0, t1);
}

// ---- point checks (Montgomery form, affine, finite)
FQ_HD fq fq_three() {
    const fq one = fq_one();
    return fq_add(fq_add(one, one), one);
}
P12_FN bool g1_on_curve(const fq &x, const fq &y) { return fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), fq_three())); }
P12_FN bool g2_on_twist(const fq2 &x, const fq2 &y) { return f_eq(f_sqr(y), f_add(f_mul(f_sqr(x), x), fq2_ld(P12_TWIST_B))); }
// membership in the order-r subgroup by its definition, [r]Q = O: double and add over the 254 bits of r with the complete Jacobian formulas
P12_FN bool g2_in_subgroup(const fq2 &x, const fq2 &y) {
    jacT<fq2> acc = jac_inf<fq2>();
#pragma unroll 1
    for (int i = 253; i >= 0; i--) {
        acc = jac_dbl(acc);
        if ((p12_r_word(i >> 5) >> (i & 31)) & 1) acc = jac_madd(acc, x, y);
    }
    return f_is_zero(acc.Z);
}
FQ_HD bool p12_words_lt_q(const u32 *w) {   // 8 standard-form words < q
    bool lt = false, eq = true;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt = lt | (eq & (w[i] < FQ_Q_H[i]));
        eq = eq & (w[i] == FQ_Q_H[i]);
    }
    return lt;
}
FQ_HD bool p12_words_zero(const u32 *w, int n) {
    u32 o = 0;
    for (int i = 0; i < n; i++) o |= w[i];
    return o == 0;
}

// One job: the Miller value of a pair of points as they cross the ABI (g1 u32[16], g2 u32[32], standard form, all-zero = infinity).
// Returns 0 computed, 1 a coordinate >= q, 2 not on its curve, 3 the G2 point outside the subgroup (not tested with P12_SKIP_SUBGROUP: the key's
// points, checked once per call).  A refused pair, and a pair with a point at infinity, still runs the fixed loop, on the generators: every job
// does the same work.  f = 1 unless the status is 0 and both points are finite
#define P12_SKIP_SUBGROUP 1u
P12_FN u32 p12_job(const u32 *g1, const u32 *g2, u32 flags, fq12 &f) {
    bool small = true;
#pragma unroll 1
    for (int k = 0; k < 2; k++) small = small & p12_words_lt_q(g1 + 8 * k);
#pragma unroll 1
    for (int k = 0; k < 4; k++) small = small & p12_words_lt_q(g2 + 8 * k);
    const bool inf1 = p12_words_zero(g1, 16), inf2 = p12_words_zero(g2, 32);
    fq xP = fq_to_mont(fq_from_words(g1)), yP = fq_to_mont(fq_from_words(g1 + 8));
    fq2 xQ = f_to_mont(FT<fq2>::from_words(g2)), yQ = f_to_mont(FT<fq2>::from_words(g2 + 16));
    u32 status = 0;
    if (!small) status = 1;
    else if ((!inf1 && !g1_on_curve(xP, yP)) || (!inf2 && !g2_on_twist(xQ, yQ))) status = 2;
    const bool sub1 = status != 0 || inf1, sub2 = status != 0 || inf2;   // compute on the generator instead
    if (sub1) {
        xP = fq_one();
        yP = fq_dbl(fq_one());
    }
    if (sub2) {
        xQ = fq2_ld(P12_G2_GEN[0]);
        yQ = fq2_ld(P12_G2_GEN[1]);
    }
    if (!(flags & P12_SKIP_SUBGROUP)) {
        const bool in = g2_in_subgroup(xQ, yQ);
        if (status == 0 && !in) {
            status = 3;
            xQ = fq2_ld(P12_G2_GEN[0]);
            yQ = fq2_ld(P12_G2_GEN[1]);
        }
    }
    p12_miller(f, xP, yP, xQ, yQ);
    if (status != 0 || inf1 || inf2) fq12_set_one(f);
    return status;
}
// One group: the product of k Miller values (108 Montgomery words each, coefficient after coefficient) and of `extra` (or NULL)
P12_FN void p12_group_product(fq12 &acc, const u32 *vals, size_t k, const u32 *extra) {
    fq12 v;
    fq12_set_one(acc);
#pragma unroll 1
    for (size_t j = 0; j <= k; j++) {
        const u32 *src = j < k ? vals + 108 * j : extra;
        if (!src) continue;
#pragma unroll 1
        for (int i = 0; i < 6; i++) v.c[i] = fq2_ld(src + 18 * i);
        fq12_mul(acc, acc, v);
    }
}
P12_FN void fq12_store(const fq12 &a, u32 *dst) {
#pragma unroll 1
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int l = 0; l < 9; l++) {
            dst[18 * i + l] = a.c[i].c0.l[l];
            dst[18 * i + 9 + l] = a.c[i].c1.l[l];
        }
}

}  // namespace
