// Corner-case operands, the exact reference and the carry / borrow classes for the Goldilocks field p = 2^64 - 2^32 + 1
// (test infrastructure, shared by gl_host_check.cpp and gl_device_check.hip).  Plain C++: nothing here comes from csrc/, so a
// defect in gl.hpp cannot hide in its own reference.  Every reference value is unsigned __int128 arithmetic with %.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>

namespace fc {
typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;

static const u64 P = 0xFFFFFFFF00000001ULL;

// ---- the reference
static inline u64 ref_mod(u128 x) { return (u64)(x % (u128)P); }
static inline u64 ref_mul(u64 a, u64 b) { return ref_mod((u128)a * b); }
static inline u64 ref_add(u64 a, u64 b) { return ref_mod((u128)a + b); }
static inline u64 ref_sub(u64 a, u64 b) { return ref_mod((u128)(a % P) + P - b % P); }
static inline u64 ref_pow(u64 b, u64 e) {
    u64 r = 1;
    b %= P;
    for (; e; e >>= 1) {
        if (e & 1) r = ref_mul(r, b);
        b = ref_mul(b, b);
    }
    return r;
}
static inline u64 ref_inv(u64 a) { return ref_pow(a, P - 2); }
static inline u64 ref_shl(u64 x, int s) { return ref_mul(x, ref_pow(2, (u64)s)); }   // x * 2^s mod p, any s >= 0

// ---- the operand set E: 518 values (duplicates stay), 450 of them canonical
static inline std::vector<u64> operands() {
    std::vector<u64> e;
    for (int k = 0; k < 64; k++) {
        const u64 b = 1ULL << k;
        const u64 v[8] = {b, b - 1, b + 1, P - b, P - b - 1, P - b + 1, ~b, (u64)0 - b};
        for (int i = 0; i < 8; i++) e.push_back(v[i]);
    }
    const u64 tail[6] = {0, P, P + 1, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFEFFFFFFFFULL, 0x7FFFFFFF00000000ULL};
    for (int i = 0; i < 6; i++) e.push_back(tail[i]);
    return e;
}
static inline std::vector<u64> canonical(const std::vector<u64> &e) {
    std::vector<u64> c;
    for (size_t i = 0; i < e.size(); i++)
        if (e[i] < P) c.push_back(e[i]);
    return c;
}
// seeds of the rarest product classes, should a refactor of E lose them: 2^48 * (2^48 + m 2^16) has L0 = L1 = 0, L3 = 1, L2 = m (class b2),
// (2^32 - 1) * (2^32 + 1) = 2^64 - 1 (class b0, H)
static inline void seed_pairs(std::vector<u64> &a, std::vector<u64> &b) {
    const u64 m[4] = {0, 1, 0x7FFF, 0xFFFF};
    for (int i = 0; i < 4; i++) {
        a.push_back(1ULL << 48);
        b.push_back((1ULL << 48) + (m[i] << 16));
    }
    a.push_back(0xFFFFFFFFULL);
    b.push_back(0x100000001ULL);
}
// n seeded values below p (splitmix64; the rejected fraction is 2^-32)
static inline std::vector<u64> random_canonical(size_t n, u64 seed) {
    std::vector<u64> v;
    u64 s = seed;
    while (v.size() < n) {
        u64 z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        if (z < P) v.push_back(z);
    }
    return v;
}
// E_c and, for every v in it, the preimage v * 2^-s mod p: a shift by s lands on the corners too
static inline std::vector<u64> with_preimages(const std::vector<u64> &ec, int s) {
    std::vector<u64> x(ec);
    const u64 back = ref_inv(ref_pow(2, (u64)s));
    for (size_t i = 0; i < ec.size(); i++) x.push_back(ref_mul(ec[i], back));
    return x;
}

// ---- product classes, from the exact integer X = a b = L0 + L1 2^32 + L2 2^64 + L3 2^96, lo = L1:L0
//   borrow  b0: lo >= L3      b1: lo < L3, (L0 - L3) mod 2^32 != 2^32 - 1      b2: lo < L3, (L0 - L3) mod 2^32 == 2^32 - 1
//   t = lo - L3 (mod 2^64), less 2^32 - 1 after a borrow;  T = t + L2 (2^32 - 1) exactly
//   fold    g0: T < p         G: T >= 2^64          H: p <= T < 2^64
enum { B0 = 0, B1 = 1, B2 = 2, G0 = 0, GG = 1, GH = 2 };
static inline int mul_class(u64 a, u64 b) {   // 3 * borrow class + fold class
    const u128 X = (u128)a * b;
    const u64 lo = (u64)X;
    const u32 L0 = (u32)lo, L2 = (u32)(X >> 64), L3 = (u32)(X >> 96);
    int bc = B0;
    u64 t = lo - L3;
    if (lo < (u64)L3) {
        bc = (u32)(L0 - L3) == 0xFFFFFFFFu ? B2 : B1;
        t -= 0xFFFFFFFFULL;
    }
    const u128 T = (u128)t + (u128)L2 * 0xFFFFFFFFULL;
    const int gc = T < (u128)P ? G0 : (T >> 64) ? GG : GH;
    return 3 * bc + gc;
}
static const char *const MUL_B[3] = {"b0", "b1", "b2"};
static const char *const MUL_G[3] = {"g0", "G", "H"};

// ---- sum classes of canonical a, b, s = a + b exactly:  A0: s < p   A1: p <= s < 2^64 (s == p counted apart)   A2: s >= 2^64
enum { A0 = 0, A1 = 1, A1P = 2, A2 = 3 };
static inline int add_class(u64 a, u64 b) {
    const u128 s = (u128)a + b;
    return s < (u128)P ? A0 : s == (u128)P ? A1P : (s >> 64) ? A2 : A1;
}
static const char *const ADD_C[4] = {"A0", "A1", "A1(s=p)", "A2"};
// ---- difference classes of canonical a, b:  D0: a >= b   D1: a < b, low word of a - b mod 2^64 != 0xFFFFFFFF   D2: ... == 0xFFFFFFFF
enum { D0 = 0, D1 = 1, D2 = 2 };
static inline int sub_class(u64 a, u64 b) { return a >= b ? D0 : (u32)(a - b) == 0xFFFFFFFFu ? D2 : D1; }
static const char *const SUB_C[3] = {"D0", "D1", "D2"};

// ---- hit counters
struct class_table {
    const char *what;
    u64 mul[9], add[4], sub[3];
    bool has_mul, has_add, has_sub;
    explicit class_table(const char *w) : what(w), has_mul(false), has_add(false), has_sub(false) {
        for (int i = 0; i < 9; i++) mul[i] = 0;
        for (int i = 0; i < 4; i++) add[i] = 0;
        for (int i = 0; i < 3; i++) sub[i] = 0;
    }
    void hit_mul(u64 a, u64 b) { has_mul = true; mul[mul_class(a, b)]++; }
    void hit_add(u64 a, u64 b) { has_add = true; add[add_class(a, b)]++; }
    void hit_sub(u64 a, u64 b) { has_sub = true; sub[sub_class(a, b)]++; }
    // one line per class, "class <what> <name> <count>"; returns the number of empty classes
    int print() const {
        int empty = 0;
        if (has_mul)
            for (int i = 0; i < 9; i++) {
                printf("class %s %s,%s %llu\n", what, MUL_B[i / 3], MUL_G[i % 3], mul[i]);
                empty += mul[i] == 0;
            }
        if (has_add)
            for (int i = 0; i < 4; i++) {
                printf("class %s %s %llu\n", what, ADD_C[i], add[i]);
                empty += add[i] == 0;
            }
        if (has_sub)
            for (int i = 0; i < 3; i++) {
                printf("class %s %s %llu\n", what, SUB_C[i], sub[i]);
                empty += sub[i] == 0;
            }
        return empty;
    }
};

// ---- one line per primitive, "prim <name> cases <n> mismatches <m>", and the first 16 mismatches in full
struct tally {
    const char *name;
    u64 cases, bad;
    explicit tally(const char *n) : name(n), cases(0), bad(0) {}
    void check(u64 got, u64 want, u64 a, u64 b, const char *cls) {
        cases++;
        if (got == want) return;
        if (bad++ < 16) printf("MISMATCH %s a=%016llx b=%016llx got=%016llx want=%016llx class=%s\n", name, a, b, got, want, cls);
    }
    u64 print() const {
        printf("prim %s cases %llu mismatches %llu\n", name, cases, bad);
        return bad;
    }
};
static inline const char *mul_class_name(u64 a, u64 b) {
    static const char *const N[9] = {"b0,g0", "b0,G", "b0,H", "b1,g0", "b1,G", "b1,H", "b2,g0", "b2,G", "b2,H"};
    return N[mul_class(a, b)];
}
}   // namespace fc
