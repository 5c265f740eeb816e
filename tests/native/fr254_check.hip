// Check of eigen_zeth_amd/csrc/fr254.hpp (F_r of BN254: nine 29-bit limbs, 64-bit column accumulators) at the operands that fill its columns
// (test infrastructure).  One source, two builds: g++ -x c++ runs every function on the host, hipcc runs a kernel per function on the GPU.
// The cases and the expected results come from a file that tests/test_field_corners.py writes with Python integers: nothing here knows how to
// multiply mod r.   usage: fr254_check CASES.bin    exit status: 0 all equal, 1 a mismatch, 2 a HIP or file error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "fr254.hpp"

enum { OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_TOMONT, OP_FROMMONT, OP_ROUNDTRIP, OP_MUL3, OP_U64, OP_DOT1, OP_DOT2, OP_DOT3, OP_DOT4, OP_DOT5, OP_DOT6, OP_COUNT };
static const char *const OP_NAME[OP_COUNT] = {"fr_add", "fr_sub", "fr_mul", "fr_sqr", "fr_to_mont", "fr_from_mont", "fr_mont_round_trip", "fr_mul3", "fr_u64_forms",
                                              "fr_dotc<1>", "fr_dotc<2>", "fr_dotc<3>", "fr_dotc<4>", "fr_dotc<5>", "fr_dotc<6>"};
struct fr_out {   // what an operation leaves: limbs, the canonical flag and the four words (zero where it has none)
    u32 r[9];
    u32 flag;
    u64 w[4];
};
struct fr_case {   // 544 bytes, the layout the Python side writes
    u32 op, pad;
    u32 x[6][9];   // up to six operands, limbs
    u32 c[54];     // fr_dotc's constants, N x 9 limbs
    u64 w[4];      // fr_from_u64's words
    fr_out want;
};
static_assert(sizeof(fr_case) == 544 && sizeof(fr_out) == 72, "layout of the case file");

template <int OP>
GL_HD void fr_apply(const fr_case &in, fr_out &out) {
    fr x[6];
    for (int n = 0; n < 6; n++)
        for (int i = 0; i < 9; i++) x[n].l[i] = in.x[n][i];
    fr r = fr_zero();
    out.flag = 0;
    for (int k = 0; k < 4; k++) out.w[k] = 0;
    if constexpr (OP == OP_ADD) r = fr_add(x[0], x[1]);
    else if constexpr (OP == OP_SUB) r = fr_sub(x[0], x[1]);
    else if constexpr (OP == OP_MUL) r = fr_mul(x[0], x[1]);
    else if constexpr (OP == OP_SQR) r = fr_sqr(x[0]);
    else if constexpr (OP == OP_TOMONT) r = fr_to_mont(x[0]);
    else if constexpr (OP == OP_FROMMONT) r = fr_from_mont(x[0]);
    else if constexpr (OP == OP_ROUNDTRIP) r = fr_from_mont(fr_to_mont(x[0]));
    else if constexpr (OP == OP_MUL3) r = fr_mul3(x[0], x[1], x[2], x[3], x[4], x[5]);
    else if constexpr (OP == OP_U64) {
        r = fr_from_u64(in.w);
        fr_to_u64(r, out.w);
        out.flag = fr_is_canonical_u64(in.w) ? 1u : 0u;
    } else r = fr_dotc<OP - OP_DOT1 + 1>(x, in.c);
    for (int i = 0; i < 9; i++) out.r[i] = r.l[i];
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
__global__ void k_fr(const fr_case *in, fr_out *out, u32 n) {   // one case per lane
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr_out o;
    fr_apply<OP>(in[i], o);
    out[i] = o;
}
static const fr_case *d_in = nullptr;
static fr_out *d_out = nullptr;
#endif

// the cases of one operation stand together in the file: [lo, hi)
template <int OP>
static void run_op(const std::vector<fr_case> &cs, std::vector<fr_out> &got, size_t lo, size_t hi) {
    if (lo == hi) return;
#if defined(__HIPCC__)
    const u32 n = (u32)(hi - lo);
    k_fr<OP><<<dim3((n + 63) / 64), 64>>>(d_in + lo, d_out + lo, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(got.data() + lo, d_out + lo, (size_t)n * sizeof(fr_out), hipMemcpyDeviceToHost));
#else
    for (size_t i = lo; i < hi; i++) fr_apply<OP>(cs[i], got[i]);
#endif
}
template <int OP>
static void run_all(const std::vector<fr_case> &cs, std::vector<fr_out> &got, const size_t *lo, const size_t *hi) {
    run_op<OP>(cs, got, lo[OP], hi[OP]);
    if constexpr (OP + 1 < OP_COUNT) run_all<OP + 1>(cs, got, lo, hi);
}

static bool below_r(const u32 *l) {   // limbs normalised: compare from the top
    for (int i = 8; i >= 0; i--)
        if (l[i] != fr_p(i)) return l[i] < fr_p(i);
    return false;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<fr_case> cs;
    fr_case c;
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
    std::vector<fr_out> got(cs.size());
    memset(got.data(), 0xA5, got.size() * sizeof(fr_out));
#if defined(__HIPCC__)
    int ndev = 0;
    CK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    CK(hipSetDevice(0));
    CK(hipMalloc((void **)&d_in, cs.size() * sizeof(fr_case)));
    CK(hipMalloc((void **)&d_out, cs.size() * sizeof(fr_out)));
    CK(hipMemcpy((void *)d_in, cs.data(), cs.size() * sizeof(fr_case), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, cs.size() * sizeof(fr_out)));
    printf("build device\n");
#else
    printf("build host\n");
#endif
    run_all<0>(cs, got, lo, hi);
    size_t total_bad = 0;
    for (int o = 0; o < OP_COUNT; o++) {
        size_t bad = 0;
        for (size_t i = lo[o]; i < hi[o]; i++) {
            const fr_out &g = got[i], &w = cs[i].want;
            bool ok = memcmp(g.r, w.r, sizeof g.r) == 0 && g.flag == w.flag && memcmp(g.w, w.w, sizeof g.w) == 0;
            for (int k = 0; k < 9; k++) ok &= g.r[k] <= FR_MASK;
            if (o != OP_U64) ok &= below_r(g.r);   // fr_from_u64 slices whatever it is given; the flag says whether that is canonical
            if (ok) continue;
            if (bad++ < 16) {
                printf("MISMATCH %s case %zu\n  got ", OP_NAME[o], i - lo[o]);
                for (int k = 8; k >= 0; k--) printf(" %08x", g.r[k]);
                printf(" flag %u\n  want", g.flag);
                for (int k = 8; k >= 0; k--) printf(" %08x", w.r[k]);
                printf(" flag %u\n  x0  ", w.flag);
                for (int k = 8; k >= 0; k--) printf(" %08x", cs[i].x[0][k]);
                printf("\n  x1  ");
                for (int k = 8; k >= 0; k--) printf(" %08x", cs[i].x[1][k]);
                printf("\n");
            }
        }
        printf("prim %s cases %zu mismatches %zu\n", OP_NAME[o], hi[o] - lo[o], bad);
        if (hi[o] == lo[o]) { printf("no case for %s\n", OP_NAME[o]); bad++; }
        total_bad += bad;
    }
#if defined(__HIPCC__)
    (void)hipFree((void *)d_in);
    (void)hipFree(d_out);
#endif
    printf("total mismatches %zu\n", total_bad);
    return total_bad ? 1 : 0;
}
