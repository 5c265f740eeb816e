// Host check of eigen_zeth_amd/csrc/gl.hpp (test infrastructure): every host-compilable function against unsigned __int128 arithmetic on the
// corner operands of field_corners.hpp -- the carry / borrow paths that uniformly random operands reach about once in 2^32 products.
// Built and run by tests/test_field_corners.py (g++, no GPU).   --random N: N seeded random canonical operands in place of E (the test
// uses it to show that random operands do not tell a mutated gl.hpp from a correct one); then no class has to be hit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gl.hpp"
#include "field_corners.hpp"

using fc::ref_add;
using fc::ref_mod;
using fc::ref_mul;
using fc::ref_sub;
typedef unsigned __int128 u128;

static std::vector<u64> E, F, Ec, Fc;   // F: the second operand stream (E itself, or a second random vector)
static bool cross = true;               // E x F, or the pairs (E[i], F[i])

template <class Fn>
static void for_pairs(const std::vector<u64> &a, const std::vector<u64> &b, Fn fn) {
    if (cross) {
        for (size_t i = 0; i < a.size(); i++)
            for (size_t j = 0; j < b.size(); j++) fn(a[i], b[j]);
    } else {
        for (size_t i = 0; i < a.size() && i < b.size(); i++) fn(a[i], b[i]);
    }
}

template <int S>
static void check_pow2(fc::tally &t, const std::vector<u64> &ec) {
    const std::vector<u64> x = fc::with_preimages(ec, S);
    for (size_t i = 0; i < x.size(); i++) t.check(gl_mul_pow2<S>(x[i]), fc::ref_shl(x[i], S), x[i], (u64)S, "-");
    if constexpr (S < 95) check_pow2<S + 1>(t, ec);
}

// the k-th product of sequence q: operands walk E with two coprime strides
static inline void seq_pair(size_t q, size_t k, u64 &a, u64 &b) {
    a = E[(q * 131 + k * 7) % E.size()];
    b = F[(q * 31 + k * 17 + 5) % F.size()];
}

// ---- cubic extension reference: schoolbook product mod x^3 - x - 1
static void ref_e3_mul(const u64 *a, const u64 *b, u64 *r) {
    u64 d[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[i + j] = ref_add(d[i + j], ref_mul(a[i], b[j]));
    // x^3 = x + 1, x^4 = x^2 + x
    r[0] = ref_add(d[0], d[3]);
    r[1] = ref_add(ref_add(d[1], d[3]), d[4]);
    r[2] = ref_add(d[2], d[4]);
}

int main(int argc, char **argv) {
    size_t nrand = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--random") && i + 1 < argc) nrand = (size_t)strtoull(argv[++i], nullptr, 10);
        else { fprintf(stderr, "usage: %s [--random N]\n", argv[0]); return 2; }
    }
    if (nrand) {
        E = fc::random_canonical(nrand, 0x5EED0001ULL);
        F = fc::random_canonical(nrand, 0x5EED0002ULL);
        cross = false;
    } else {
        E = fc::operands();
        F = E;
    }
    Ec = fc::canonical(E);
    Fc = fc::canonical(F);
    printf("operands %zu canonical %zu mode %s\n", E.size(), Ec.size(), nrand ? "random" : "corners");
    u64 bad = 0;
    int empty = 0;

    {   // canonicalisation, negation
        fc::tally tc("gl_canon"), tn("gl_neg");
        for (size_t i = 0; i < E.size(); i++) tc.check(gl_canon(E[i]), E[i] % fc::P, E[i], 0, "-");
        for (size_t i = 0; i < Ec.size(); i++) tn.check(gl_neg(Ec[i]), ref_sub(0, Ec[i]), Ec[i], 0, "-");
        bad += tc.print() + tn.print();
    }
    {   // sums and differences of canonical values
        fc::tally ta("gl_add"), ts("gl_sub"), tw("gl_add_weak");
        fc::class_table ca("add"), cs("sub");
        for_pairs(Ec, Fc, [&](u64 a, u64 b) {
            ta.check(gl_add(a, b), ref_add(a, b), a, b, fc::ADD_C[fc::add_class(a, b)]);
            ts.check(gl_sub(a, b), ref_sub(a, b), a, b, fc::SUB_C[fc::sub_class(a, b)]);
            ca.hit_add(a, b);
            cs.hit_sub(a, b);
        });
        for_pairs(E, Fc, [&](u64 a, u64 b) { tw.check(gl_add_weak(a, b) % fc::P, ref_add(a % fc::P, b), a, b, "-"); });   // any u64 + canonical
        bad += ta.print() + ts.print() + tw.print();
        empty += ca.print() + cs.print();
    }
    {   // lo + hl 2^64 + hh 2^96
        fc::tally tr("gl_reduce96"), tw("gl_reduce96_weak");
        const u32 H[7] = {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
        const size_t n = nrand ? E.size() / 8 + 1 : E.size();
        for (size_t i = 0; i < n && i < E.size(); i++)
            for (int j = 0; j < 7; j++)
                for (int k = 0; k < 7; k++) {
                    // 2^96 == -1: lo + hl 2^64 - hh, kept non-negative by adding p
                    const u64 want = ref_mod((u128)E[i] + ((u128)H[j] << 64) + (u128)fc::P - H[k]);
                    tr.check(gl_reduce96(E[i], H[j], H[k]), want, E[i], ((u64)H[k] << 32) | H[j], "-");
                    tw.check(gl_reduce96_weak(E[i], H[j], H[k]) % fc::P, want, E[i], ((u64)H[k] << 32) | H[j], "-");
                }
        bad += tr.print() + tw.print();
    }
    {   // products of any two u64
        fc::tally tm("gl_mul"), tw("gl_mul_weak"), tq("gl_sqr");
        fc::class_table cm("mul");
        for_pairs(E, F, [&](u64 a, u64 b) {
            const u64 want = ref_mul(a, b);
            const char *cls = fc::mul_class_name(a, b);
            tm.check(gl_mul(a, b), want, a, b, cls);
            tw.check(gl_mul_weak(a, b) % fc::P, want, a, b, cls);
            cm.hit_mul(a, b);
        });
        for (size_t i = 0; i < E.size(); i++) tq.check(gl_sqr(E[i]), ref_mul(E[i], E[i]), E[i], E[i], fc::mul_class_name(E[i], E[i]));
        if (!nrand) {   // the seed families of the rarest classes, whatever becomes of E
            std::vector<u64> sa, sb;
            fc::seed_pairs(sa, sb);
            for (size_t i = 0; i < sa.size(); i++) {
                tm.check(gl_mul(sa[i], sb[i]), ref_mul(sa[i], sb[i]), sa[i], sb[i], fc::mul_class_name(sa[i], sb[i]));
                const int want_cls = i + 1 < sa.size() ? fc::B2 : 3 * fc::B0 + fc::GH;
                const int cls = i + 1 < sa.size() ? fc::mul_class(sa[i], sb[i]) / 3 : fc::mul_class(sa[i], sb[i]);
                tm.check((u64)cls, (u64)want_cls, sa[i], sb[i], "class of a seed pair");
            }
        }
        bad += tm.print() + tw.print() + tq.print();
        empty += cm.print();
    }
    {   // x 2^S, S = 1..95, on the corners and on what a shift sends to them
        fc::tally tp("gl_mul_pow2");
        std::vector<u64> ec(Ec);
        if (nrand && ec.size() > nrand / 64 + 1) ec.resize(nrand / 64 + 1);
        check_pow2<1>(tp, ec);
        bad += tp.print();
    }
    {   // the unreduced accumulator
        fc::tally tk("gl_acc");
        const size_t LEN[5] = {1, 2, 3, 17, 4096};
        for (int l = 0; l < 5; l++)
            for (size_t q = 0; q < 64; q++) {
                gl_acc s = gl_acc_zero();
                u64 want = 0, a = 0, b = 0;
                for (size_t k = 0; k < LEN[l]; k++) {
                    seq_pair(q * 5 + l, k, a, b);
                    gl_acc_mac(s, a, b);
                    want = ref_add(want, ref_mul(a, b));
                }
                tk.check(gl_acc_reduce(s), want, a, b, "-");
            }
        if (!nrand) {   // the largest sums: 4096 times the same maximal product
            const u64 M[4] = {0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFEFFFFFFFFULL, fc::P - 1, 0xFFFFFFFF80000000ULL};
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    gl_acc s = gl_acc_zero();
                    for (int k = 0; k < 4096; k++) gl_acc_mac(s, M[i], M[j]);
                    tk.check(gl_acc_reduce(s), ref_mul(4096, ref_mul(M[i], M[j])), M[i], M[j], "-");
                }
        }
        bad += tk.print();
    }
    {   // powers and inverses
        fc::tally tp("gl_pow"), ti("gl_inv");
        const size_t nb = Ec.size() < 4096 ? Ec.size() : 4096;   // bases; 64 exponents each, walking E
        for (size_t i = 0; i < nb; i++)
            for (size_t k = 0; k < 64; k++) {
                const u64 e = E[(i + k * 67) % E.size()];
                tp.check(gl_pow(Ec[i], e), fc::ref_pow(Ec[i], e), Ec[i], e, "-");
            }
        for (size_t i = 0; i < nb; i++) {
            if (Ec[i] == 0) continue;
            const u64 v = gl_inv(Ec[i]);
            ti.check(ref_mul(v, Ec[i]), 1, Ec[i], v, "a*inv");
            ti.check(v, fc::ref_inv(Ec[i]), Ec[i], 0, "-");
        }
        ti.check(gl_inv(0), 0, 0, 0, "inv(0) = 0^(p-2) = 0");
        bad += tp.print() + ti.print();
    }
    {   // cubic extension: components over 16 canonical corners
        fc::tally tm("e3_mul"), ta("e3_adj"), ti("e3_inv");
        u64 c[16];
        if (nrand) {
            for (int i = 0; i < 16; i++) c[i] = Ec[i];
        } else {
            const u64 pick[16] = {0, 1, 2, fc::P - 1, fc::P - 2, 0xFFFFFFFFULL, 0x100000000ULL, 0x100000001ULL, 0xFFFFFFFE00000001ULL, 0xFFFFFFFEFFFFFFFFULL,
                                  0x7FFFFFFF00000000ULL, 0x8000000000000000ULL, 0x7FFFFFFFFFFFFFFFULL, 0xFFFFFFFE00000002ULL, 1ULL << 48, 0xFFFEFFFF00000001ULL};
            for (int i = 0; i < 16; i++) {   // every one of them is in E_c
                c[i] = pick[i];
                bool in = false;
                for (size_t k = 0; k < Ec.size(); k++) in |= Ec[k] == c[i];
                tm.check(in, 1, c[i], 0, "component not in E_c");
            }
        }
        const u64 one[3] = {1, 0, 0};
        for (int i = 0; i < 4096; i++) {
            const u64 x[3] = {c[i & 15], c[(i >> 4) & 15], c[i >> 8]};
            const e3 X = e3_make(x[0], x[1], x[2]);
            for (int j = i % 61; j < 4096; j += 61) {
                const u64 y[3] = {c[j & 15], c[(j >> 4) & 15], c[j >> 8]};
                u64 want[3];
                ref_e3_mul(x, y, want);
                const e3 got = e3_mul(X, e3_make(y[0], y[1], y[2]));
                for (int k = 0; k < 3; k++) tm.check(got.c[k], want[k], (u64)i, (u64)j, "component index pair");
            }
            u64 det, prod[3];
            const e3 adj = e3_adj(X, &det);
            ref_e3_mul(x, adj.c, prod);   // x adj(x) = det
            ta.check(prod[0], det, (u64)i, 0, "x*adj c0 = det");
            ta.check(prod[1], 0, (u64)i, 1, "x*adj c1 = 0");
            ta.check(prod[2], 0, (u64)i, 2, "x*adj c2 = 0");
            if (i == 0 && !nrand) { ta.check(det, 0, 0, 0, "det(0)"); continue; }
            const e3 inv = e3_inv(X);
            ref_e3_mul(x, inv.c, prod);
            for (int k = 0; k < 3; k++) ti.check(prod[k], one[k], (u64)i, (u64)k, "x*inv = 1");
        }
        bad += tm.print() + ta.print() + ti.print();
    }
    printf("total mismatches %llu empty classes %d\n", bad, nrand ? 0 : empty);
    return (bad != 0 || (!nrand && empty != 0)) ? 1 : 0;
}
