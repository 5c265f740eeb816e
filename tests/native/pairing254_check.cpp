// Runs the functions of eigen_zeth_amd/csrc/pairing254.hpp (the Fermat inverse in F_q and F_q2, F_q12, the Miller loop, the final exponentiation,
// the point checks) on the cases of a file and writes what they return, every word as stored (test infrastructure).  A host program (g++).
// The program judges nothing: tests/test_pairing254.py writes the cases and compares every raw result with Python integers and the checker's pairing.
//   usage: pairing254_check CASES.bin RESULTS.bin      exit status: 0 done, 2 a file or usage error
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
// the headers mark their functions for hipcc; a host compiler reads the same bodies as plain functions
#define __host__
#define __device__
#define __forceinline__ inline
#define CHK_FN inline
#include "pairing254.hpp"

enum { OP_FQINV, OP_F2INV, OP_MUL, OP_SQR, OP_MULLINE, OP_INV, OP_CONJ, OP_FROB1, OP_FROB2, OP_FROB3, OP_FINALEXP, OP_PAIRING, OP_SUBGROUP, OP_COUNT };
static const char *const OP_NAME[OP_COUNT] = {"fq_inv", "fq2_inv", "fq12_mul", "fq12_sqr", "fq12_mul_line", "fq12_inv", "fq12_conj", "fq12_frob1",
                                              "fq12_frob2", "fq12_frob3", "fq12_final_exp", "pairing", "g2_checks"};
// operands: F_q12 elements are twelve flat-basis coefficients of nine Montgomery limbs; a line is x[1][0..54) = l0, l1, l3 (F_q2, 18 limbs each);
// points are standard-form words: x[0][0..16) a G1 point, x[0][16..48) (pairing) or x[0][0..32) (g2_checks) a G2 point
struct p12_case {
    u32 op, flags;
    u32 x[2][108];
};
struct p12_out {   // r: the result in the operand's form; flag: a status or the checks' bits; w: GT words (final_exp, pairing)
    u32 r[108];
    u32 flag;
    u32 w[96];
};
static_assert(sizeof(p12_case) == 872 && sizeof(p12_out) == 820, "layout of the case and result files");

CHK_FN void p12_apply(const p12_case &in, p12_out &out) {
    fq12 a, b;
    switch (in.op) {
        case OP_FQINV: {
            const fq r = fq_inv(fq_ld(in.x[0]));
            for (int i = 0; i < 9; i++) out.r[i] = r.l[i];
            break;
        }
        case OP_F2INV: {
            const fq2 r = fq2_inv(fq2_ld(in.x[0]));
            for (int i = 0; i < 9; i++) { out.r[i] = r.c0.l[i]; out.r[9 + i] = r.c1.l[i]; }
            break;
        }
        case OP_MUL:
            fq12_from_flat(a, in.x[0]);
            fq12_from_flat(b, in.x[1]);
            fq12_mul(a, a, b);
            fq12_to_flat(a, out.r);
            break;
        case OP_SQR:
            fq12_from_flat(a, in.x[0]);
            fq12_sqr(a, a);
            fq12_to_flat(a, out.r);
            break;
        case OP_MULLINE:
            fq12_from_flat(a, in.x[0]);
            fq12_mul_line(a, a, fq2_ld(in.x[1]), fq2_ld(in.x[1] + 18), fq2_ld(in.x[1] + 36));
            fq12_to_flat(a, out.r);
            break;
        case OP_INV:
            fq12_from_flat(a, in.x[0]);
            fq12_inv(b, a);
            fq12_to_flat(b, out.r);
            break;
        case OP_CONJ:
            fq12_from_flat(a, in.x[0]);
            fq12_conj(b, a);
            fq12_to_flat(b, out.r);
            break;
        case OP_FROB1:
        case OP_FROB2:
        case OP_FROB3:
            fq12_from_flat(a, in.x[0]);
            fq12_frob(b, a, (int)in.op - OP_FROB1 + 1);
            fq12_to_flat(b, out.r);
            break;
        case OP_FINALEXP:
            fq12_from_flat(a, in.x[0]);
            fq12_final_exp(b, a);
            fq12_to_flat(b, out.r);
            fq12_to_flat_words(b, out.w);
            break;
        case OP_PAIRING:
            out.flag = p12_job(in.x[0], in.x[0] + 16, in.flags, a);
            fq12_final_exp(b, a);
            fq12_to_flat_words(b, out.w);
            break;
        default: {
            const fq2 x = f_to_mont(FT<fq2>::from_words(in.x[0])), y = f_to_mont(FT<fq2>::from_words(in.x[0] + 16));
            out.flag = (g2_on_twist(x, y) ? 1u : 0u) | (g2_in_subgroup(x, y) ? 2u : 0u);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASES.bin RESULTS.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<p12_case> cs;
    p12_case c;
    while (fread(&c, sizeof c, 1, f) == 1) cs.push_back(c);
    fclose(f);
    if (cs.empty()) { fprintf(stderr, "no cases in %s\n", argv[1]); return 2; }
    size_t count[OP_COUNT] = {0};
    for (size_t i = 0; i < cs.size(); i++) {
        if (cs[i].op >= OP_COUNT) { fprintf(stderr, "case %zu: unknown operation\n", i); return 2; }
        count[cs[i].op]++;
    }
    std::vector<p12_out> got(cs.size());
    memset(got.data(), 0, got.size() * sizeof(p12_out));
    printf("build host\n");
    for (size_t i = 0; i < cs.size(); i++) p12_apply(cs[i], got[i]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(got.data(), sizeof(p12_out), got.size(), f) != got.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int o = 0; o < OP_COUNT; o++) printf("prim %s cases %zu\n", OP_NAME[o], count[o]);
    return 0;
}
