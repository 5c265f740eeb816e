// Runs every function of eigen_zeth_amd/csrc/fq254.hpp (BN254 F_q and F_q2 on nine 29-bit limbs, the lazy forms of the G1 bucket sums, the
// Jacobian formulas over both fields) on the cases of a file and writes what they return, every word as stored (test infrastructure).
// One source, two builds: g++ -x c++ runs the cases on the host, hipcc runs one case per lane on the GPU.  The program judges nothing:
// tests/test_fq254.py writes the cases and compares every raw result with Python integers, so no function here vouches for another.
//   usage: fq254_check CASES.bin RESULTS.bin      exit status: 0 done, 2 a HIP, file or usage error
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CHK_FN __device__ inline
#else
// the header marks its functions for hipcc; a host compiler reads the same bodies as plain inline functions
#define __host__
#define __device__
#define __forceinline__ inline
#define CHK_FN inline
#endif
#include "fq254.hpp"

enum {
    OP_ADD, OP_SUB, OP_DBL, OP_MUL, OP_SQR, OP_TOMONT, OP_FROMMONT, OP_ROUNDTRIP, OP_FROMWORDS, OP_WORDS_RT, OP_ZERO_EQ, OP_NORMSUB, OP_NEGLAZY, OP_MUL2,
    OP_F2MUL, OP_F2SQR, OP_F2ADD, OP_F2SUB, OP_F2DBL, OP_INV, OP_F2INV,
    OP_LZMUL, OP_LZSUB1, OP_LZSUB3, OP_LZSUB5, OP_LZSUB6, OP_LZSUB7, OP_LZSUB2_4, OP_LZADD, OP_LZDBL, OP_LZQUAD, OP_LZCANON, OP_LZISZERO,
    OP_G1DBL, OP_G1MADD, OP_G1ADD, OP_G1MULSMALL, OP_G2DBL, OP_G2MADD, OP_G2ADD, OP_G2MULSMALL, OP_MADDLAZY, OP_CHAIN, OP_COUNT
};
static const char *const OP_NAME[OP_COUNT] = {
    "fq_add", "fq_sub", "fq_dbl", "fq_mul", "fq_sqr", "fq_to_mont", "fq_from_mont", "fq_mont_round_trip", "fq_from_words", "fq_words_round_trip", "fq_is_zero_eq",
    "fq_norm_sub", "fq_neg_lazy", "fq_mul2", "f2_mul", "f2_sqr", "f2_add", "f2_sub", "f2_dbl", "fq_inv_host", "f2_inv_host",
    "lz_mul", "lz_sub<1>", "lz_sub<3>", "lz_sub<5>", "lz_sub<6>", "lz_sub<7>", "lz_sub2<4>", "lz_add", "lz_dbl", "lz_quad", "lz_canon", "lz_is_zero_mod_q",
    "g1_jac_dbl", "g1_jac_madd", "g1_jac_add", "g1_jac_mul_small", "g2_jac_dbl", "g2_jac_madd", "g2_jac_add", "g2_jac_mul_small", "jac_madd_lazy", "jac_madd_lazy_chain"};
struct fq_case {   // 472 bytes, the layout the Python side writes
    u32 op, k;     // k: jac_mul_small's factor, or 1 where the bucket kernel would negate the affine point
    u32 x[12][9];  // operands, limbs as the function takes them
    u32 w[8];      // fq_from_words' words
};
struct fq_out {    // 360 bytes: up to nine field elements, a flag and eight words; what an operation does not write stays zero
    u32 r[9][9];
    u32 flag;
    u32 w[8];
};
static_assert(sizeof(fq_case) == 472 && sizeof(fq_out) == 360, "layout of the case and result files");

CHK_FN fq ld(const fq_case &in, int n) {
    fq a;
    for (int i = 0; i < 9; i++) a.l[i] = in.x[n][i];
    return a;
}
CHK_FN fq2 ld2(const fq_case &in, int n) { return fq2_make(ld(in, n), ld(in, n + 1)); }
CHK_FN void st(fq_out &out, int n, const fq &a) {
    for (int i = 0; i < 9; i++) out.r[n][i] = a.l[i];
}
CHK_FN void st(fq_out &out, int n, const fq2 &a) {
    st(out, n, a.c0);
    st(out, n + 1, a.c1);
}
template <class F> struct NF;   // field elements of F in units of fq
template <> struct NF<fq> { static constexpr int N = 1; };
template <> struct NF<fq2> { static constexpr int N = 2; };
CHK_FN fq ldF(const fq_case &in, int n, fq *) { return ld(in, n); }
CHK_FN fq2 ldF(const fq_case &in, int n, fq2 *) { return ld2(in, 2 * n); }
template <class F>
CHK_FN jacT<F> ldj(const fq_case &in, int n) {   // the n-th F element onwards: X, Y, Z
    jacT<F> p;
    p.X = ldF(in, n, (F *)nullptr);
    p.Y = ldF(in, n + 1, (F *)nullptr);
    p.Z = ldF(in, n + 2, (F *)nullptr);
    return p;
}
template <class F>
CHK_FN void stj(fq_out &out, int n, const jacT<F> &p) {
    st(out, n * NF<F>::N, p.X);
    st(out, (n + 1) * NF<F>::N, p.Y);
    st(out, (n + 2) * NF<F>::N, p.Z);
}
template <class F, int OP>
CHK_FN void curve_apply(const fq_case &in, fq_out &out) {
    const jacT<F> p = ldj<F>(in, 0);
    if constexpr (OP == 0) stj(out, 0, jac_dbl(p));
    else if constexpr (OP == 1) stj(out, 0, jac_madd(p, ldF(in, 3, (F *)nullptr), ldF(in, 4, (F *)nullptr)));
    else if constexpr (OP == 2) stj(out, 0, jac_add(p, ldj<F>(in, 3)));
    else stj(out, 0, jac_mul_small(p, in.k));
}
// the affine point as the bucket kernel hands it over (madd_packed): a negative digit adds (x, q - y), formed with lz_sub<1>
CHK_FN jacT<fq> madd_lazy_as_packed(const jacT<fq> &acc, const fq &x, fq y, u32 neg) {
    if (neg) y = lz_sub<1>(fq_zero(), y);
    return jac_madd_lazy(acc, x, y);
}

template <int OP>
CHK_FN void fq_apply(const fq_case &in, fq_out &out) {
    const fq a = ld(in, 0), b = ld(in, 1);
    if constexpr (OP == OP_ADD) st(out, 0, fq_add(a, b));
    else if constexpr (OP == OP_SUB) st(out, 0, fq_sub(a, b));
    else if constexpr (OP == OP_DBL) st(out, 0, fq_dbl(a));
    else if constexpr (OP == OP_MUL) st(out, 0, fq_mul(a, b));
    else if constexpr (OP == OP_SQR) st(out, 0, fq_sqr(a));
    else if constexpr (OP == OP_TOMONT) st(out, 0, fq_to_mont(a));
    else if constexpr (OP == OP_FROMMONT) st(out, 0, fq_from_mont(a));
    else if constexpr (OP == OP_ROUNDTRIP) st(out, 0, fq_from_mont(fq_to_mont(a)));
    else if constexpr (OP == OP_FROMWORDS) {
        const fq r = fq_from_words(in.w);
        st(out, 0, r);
        fq_to_words(r, out.w);
    } else if constexpr (OP == OP_WORDS_RT) {
        fq_to_words(a, out.w);
        st(out, 0, fq_from_words(out.w));
    } else if constexpr (OP == OP_ZERO_EQ) out.flag = (fq_is_zero(a) ? 1u : 0u) | (fq_eq(a, b) ? 2u : 0u);
    else if constexpr (OP == OP_NORMSUB) st(out, 0, fq_norm_sub(in.x[0]));
    else if constexpr (OP == OP_NEGLAZY) st(out, 0, fq_neg_lazy(a));
    else if constexpr (OP == OP_MUL2) st(out, 0, fq_mul2(a, b, ld(in, 2), ld(in, 3)));
    else if constexpr (OP == OP_F2MUL) st(out, 0, f_mul(ld2(in, 0), ld2(in, 2)));
    else if constexpr (OP == OP_F2SQR) st(out, 0, f_sqr(ld2(in, 0)));
    else if constexpr (OP == OP_F2ADD) st(out, 0, f_add(ld2(in, 0), ld2(in, 2)));
    else if constexpr (OP == OP_F2SUB) st(out, 0, f_sub(ld2(in, 0), ld2(in, 2)));
    else if constexpr (OP == OP_F2DBL) st(out, 0, f_dbl(ld2(in, 0)));
#if !defined(__HIPCC__)
    else if constexpr (OP == OP_INV) st(out, 0, fq_inv_host(a));
    else if constexpr (OP == OP_F2INV) st(out, 0, f_inv_host(ld2(in, 0)));
#endif
    else if constexpr (OP == OP_LZMUL) st(out, 0, lz_mul(a, b));
    else if constexpr (OP == OP_LZSUB1) st(out, 0, lz_sub<1>(a, b));
    else if constexpr (OP == OP_LZSUB3) st(out, 0, lz_sub<3>(a, b));
    else if constexpr (OP == OP_LZSUB5) st(out, 0, lz_sub<5>(a, b));
    else if constexpr (OP == OP_LZSUB6) st(out, 0, lz_sub<6>(a, b));
    else if constexpr (OP == OP_LZSUB7) st(out, 0, lz_sub<7>(a, b));
    else if constexpr (OP == OP_LZSUB2_4) st(out, 0, lz_sub2<4>(a, b, ld(in, 2)));
    else if constexpr (OP == OP_LZADD) st(out, 0, lz_add(a, b));
    else if constexpr (OP == OP_LZDBL) st(out, 0, lz_dbl(a));
    else if constexpr (OP == OP_LZQUAD) st(out, 0, lz_quad(a));
    else if constexpr (OP == OP_LZCANON) st(out, 0, lz_canon(a));
    else if constexpr (OP == OP_LZISZERO) out.flag = lz_is_zero_mod_q(a) ? 1u : 0u;
    else if constexpr (OP >= OP_G1DBL && OP <= OP_G1MULSMALL) curve_apply<fq, OP - OP_G1DBL>(in, out);
    else if constexpr (OP >= OP_G2DBL && OP <= OP_G2MULSMALL) curve_apply<fq2, OP - OP_G2DBL>(in, out);
    else if constexpr (OP == OP_MADDLAZY) {
        const jacT<fq> r = madd_lazy_as_packed(ldj<fq>(in, 0), ld(in, 3), ld(in, 4), in.k);
        stj(out, 0, r);
        stj(out, 3, jac_canon(r));
    }
}
// the cases of OP_CHAIN are the steps of ONE accumulation from infinity, in file order: every intermediate is stored
CHK_FN void chain_apply(const fq_case *in, fq_out *out, u32 n) {
    jacT<fq> acc = jac_inf<fq>();
    for (u32 i = 0; i < n; i++) {
        acc = madd_lazy_as_packed(acc, ld(in[i], 3), ld(in[i], 4), in[i].k);
        stj(out[i], 0, acc);
        stj(out[i], 3, jac_canon(acc));
    }
}

#if defined(__HIPCC__)
#define CK(x)                                                                                   \
    do {                                                                                        \
        const hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            fflush(stdout);                                                                     \
            exit(2);                                                                            \
        }                                                                                       \
    } while (0)
template <int OP>
__global__ void k_fq(const fq_case *in, fq_out *out, u32 n) {   // one case per lane
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fq_out o;
    memset(&o, 0, sizeof o);
    fq_apply<OP>(in[i], o);
    out[i] = o;
}
__global__ void k_chain(const fq_case *in, fq_out *out, u32 n) {   // one lane walks the whole chain
    if (blockIdx.x == 0 && threadIdx.x == 0) chain_apply(in, out, n);
}
static const fq_case *d_in = nullptr;
static fq_out *d_out = nullptr;
#endif

// the cases of one operation stand together in the file: [lo, hi)
template <int OP>
static void run_op(const std::vector<fq_case> &cs, std::vector<fq_out> &got, size_t lo, size_t hi) {
    if (lo == hi) return;
#if defined(__HIPCC__)
    if (OP == OP_INV || OP == OP_F2INV) { fprintf(stderr, "%s is host code: no such case in a device run\n", OP_NAME[OP]); exit(2); }
    const u32 n = (u32)(hi - lo);
    if constexpr (OP == OP_CHAIN) k_chain<<<1, 64>>>(d_in + lo, d_out + lo, n);
    else k_fq<OP><<<dim3((n + 63) / 64), 64>>>(d_in + lo, d_out + lo, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(got.data() + lo, d_out + lo, (size_t)n * sizeof(fq_out), hipMemcpyDeviceToHost));
#else
    if constexpr (OP == OP_CHAIN) chain_apply(cs.data() + lo, got.data() + lo, (u32)(hi - lo));
    else
        for (size_t i = lo; i < hi; i++) fq_apply<OP>(cs[i], got[i]);
#endif
}
template <int OP>
static void run_all(const std::vector<fq_case> &cs, std::vector<fq_out> &got, const size_t *lo, const size_t *hi) {
    run_op<OP>(cs, got, lo[OP], hi[OP]);
    if constexpr (OP + 1 < OP_COUNT) run_all<OP + 1>(cs, got, lo, hi);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASES.bin RESULTS.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<fq_case> cs;
    fq_case c;
    while (fread(&c, sizeof c, 1, f) == 1) cs.push_back(c);
    fclose(f);
    if (cs.empty()) { fprintf(stderr, "no cases in %s\n", argv[1]); return 2; }
    size_t lo[OP_COUNT], hi[OP_COUNT];
    for (int o = 0; o < OP_COUNT; o++) lo[o] = hi[o] = 0;
    for (size_t i = 0; i < cs.size(); i++) {
        const u32 o = cs[i].op;
        if (o >= OP_COUNT || (i && cs[i - 1].op > o)) { fprintf(stderr, "case %zu: operations must be known and ascending\n", i); return 2; }
        if (lo[o] == hi[o]) lo[o] = i;
        hi[o] = i + 1;
    }
    std::vector<fq_out> got(cs.size());
    memset(got.data(), 0, got.size() * sizeof(fq_out));
#if defined(__HIPCC__)
    int ndev = 0;
    CK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    CK(hipSetDevice(0));
    CK(hipMalloc((void **)&d_in, cs.size() * sizeof(fq_case)));
    CK(hipMalloc((void **)&d_out, cs.size() * sizeof(fq_out)));
    CK(hipMemcpy((void *)d_in, cs.data(), cs.size() * sizeof(fq_case), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0, cs.size() * sizeof(fq_out)));
    printf("build device\n");
#else
    printf("build host\n");
#endif
    run_all<0>(cs, got, lo, hi);
#if defined(__HIPCC__)
    (void)hipFree((void *)d_in);
    (void)hipFree(d_out);
#endif
    f = fopen(argv[2], "wb");
    if (!f || fwrite(got.data(), sizeof(fq_out), got.size(), f) != got.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int o = 0; o < OP_COUNT; o++) printf("prim %s cases %zu\n", OP_NAME[o], hi[o] - lo[o]);
    return 0;
}
