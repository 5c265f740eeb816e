// F_r of BN254 on the HOST: four 64-bit limbs, Montgomery form with R = 2^256 -- what the R1CS evaluator, the witness programs and the key
// generator (csrc/r1cs_host.hip) compute in on the request path of GenFinalProof.  Same function names as the nine-limb `fr` of fr254.hpp (the
// device's layout, also usable on the host), as overloads: on a CPU with a 64 x 64 multiplier this form is several times faster.
// Host only; builds as plain C++.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fr254.hpp"

typedef unsigned __int128 u128;
// (the C ABI's uint64_t and gl.hpp's u64 are distinct types of one size: the one cast)
inline bool fr_is_canonical_u64(const uint64_t *w) { return fr_is_canonical_u64((const u64 *)w); }

namespace {      // (per translation unit, as csrc/fq254.hpp: the compiler inlines these into the few loops that use them)

struct Fr { uint64_t l[4]; };
const uint64_t FR_MOD[4] = FR_MODULUS_U64;
const Fr FR_R2 = {{0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL}};
const Fr FR_ONE = {{0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL}};
const uint64_t FR_N0 = 0xc2e1f593efffffffULL;   // -r^-1 mod 2^64

inline bool fr_geq_mod(const uint64_t *a) {
    for (int i = 3; i >= 0; i--) {
        if (a[i] > FR_MOD[i]) return true;
        if (a[i] < FR_MOD[i]) return false;
    }
    return true;
}
inline void fr_sub_mod(uint64_t *a) {
    u128 b = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a[i] - FR_MOD[i] - (uint64_t)b;
        a[i] = (uint64_t)d;
        b = (d >> 64) & 1;
    }
}
inline Fr fr_add(const Fr &a, const Fr &b) {
    Fr r;
    u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)a.l[i] + b.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
    if (c || fr_geq_mod(r.l)) fr_sub_mod(r.l);
    return r;
}
inline Fr fr_sub(const Fr &a, const Fr &b) {
    Fr r;
    u128 br = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.l[i] - b.l[i] - (uint64_t)br;
        r.l[i] = (uint64_t)d;
        br = (d >> 64) & 1;
    }
    if (br) {
        u128 c = 0;
        for (int i = 0; i < 4; i++) { c += (u128)r.l[i] + FR_MOD[i]; r.l[i] = (uint64_t)c; c >>= 64; }
    }
    return r;
}
// CIOS Montgomery product.  Always inlined: the row loops are made of it, and with a constant operand (fr_to_std's 1) most of it folds away
__attribute__((always_inline)) inline Fr fr_mul(const Fr &a, const Fr &b) {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) { c += (u128)a.l[j] * b.l[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * FR_N0;
        c = (u128)m * FR_MOD[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; j++) { c += (u128)m * FR_MOD[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fr r = {{t[0], t[1], t[2], t[3]}};
    if (t[4] || fr_geq_mod(r.l)) fr_sub_mod(r.l);
    return r;
}
// the coefficient 1 as a type of its own: a walk over the terms of a linear combination hands it out where the blob stores none, and
// fr_mul(coefficient, x) costs nothing there
struct FrUnit {};
inline const Fr &fr_mul(FrUnit, const Fr &x) { return x; }
inline bool fr_is_zero(const Fr &a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
inline bool fr_eq(const Fr &a, const Fr &b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }
inline Fr fr_from_std(const uint64_t *w) { Fr a = {{w[0], w[1], w[2], w[3]}}; return fr_mul(a, FR_R2); }
inline void fr_to_std(const Fr &a, uint64_t *w) { const Fr one = {{1, 0, 0, 0}}; const Fr r = fr_mul(a, one); memcpy(w, r.l, 32); }
inline Fr fr_pow(Fr a, const uint64_t *e, int bits) {
    Fr r = FR_ONE;
    for (int i = bits - 1; i >= 0; i--) {
        r = fr_mul(r, r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = fr_mul(r, a);
    }
    return r;
}
inline Fr fr_inv(const Fr &a) {
    uint64_t e[4] = {FR_MOD[0] - 2, FR_MOD[1], FR_MOD[2], FR_MOD[3]};
    return fr_pow(a, e, 254);
}
// the primitive 2^k-th root of unity 5^((r - 1) / 2^k), k <= 28 (the snarkjs / circom convention)
inline Fr fr_root_of_unity(unsigned k) {
    uint64_t e[4] = {FR_MOD[0] - 1, FR_MOD[1], FR_MOD[2], FR_MOD[3]};
    for (unsigned s = 0; s < k; s++)
        for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i < 3 ? e[i + 1] << 63 : 0);
    const uint64_t five[4] = {5, 0, 0, 0};
    return fr_pow(fr_from_std(five), e, 254);
}

}  // namespace
