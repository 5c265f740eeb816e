// The stage-2 witness columns of a STARK: a running product or sum over the rows of the trace, in F_{p^3}, made at the challenge g.
//   grand product (permutation argument):  Z[0] = 1,  Z[i+1] = Z[i] * (a[i] + g) / (b[i] + g);  out planes u64[3][N]
//   LogUp (range check / lookup):  h1 = 1/(a+g), h2 = m/(t+g), S[0] = 0, S[i+1] = S[i] + h1[i] - h2[i];  planes h1 0..2, h2 3..5, S 6..8
// Both are ONE exclusive scan, written once over a monoid (E3Mul / E3Add) and an argument that supplies what a row stores, the term it
// contributes and the planes the running value lives in.  Three launches: (1) the terms, the exclusive scan inside each lane's GP_PER rows
// and of the lanes of a block (LDS), one total per block;  (2) exclusive scan of the block totals (one workgroup);  (3) the block offsets.
// Below them: the walk over a program's stage-2 table, which every prover and every witness check goes through, so that their columns are the same.
#include <hip/hip_runtime.h>

#include "ctx.hpp"

namespace {

#define GP_PER 16
#define GP_BLK 256

struct E3Mul {
    static __device__ __forceinline__ e3 id() { return e3_make(1, 0, 0); }
    static __device__ __forceinline__ e3 op(e3 a, e3 b) { return e3_mul(a, b); }
};
struct E3Add {
    static __device__ __forceinline__ e3 id() { return e3_make(0, 0, 0); }
    static __device__ __forceinline__ e3 op(e3 a, e3 b) { return e3_add(a, b); }
};

template <class Arg>
__device__ __forceinline__ e3 running_get(const Arg &A, u64 i) {
    return e3_make(A.out[(u64)Arg::PLANE * A.n + i], A.out[(u64)(Arg::PLANE + 1) * A.n + i], A.out[(u64)(Arg::PLANE + 2) * A.n + i]);
}
template <class Arg>
__device__ __forceinline__ void running_put(const Arg &A, u64 i, e3 v) {
#pragma unroll
    for (int c = 0; c < 3; c++) A.out[(u64)(Arg::PLANE + c) * A.n + i] = v.c[c];
}

// an argument: typedef M (the monoid), PLANE (first of the three planes of the running value), out / totals / g / n, and row(i, acc): stores row i
// -- the running value acc and whatever else the argument keeps per row -- and returns the term the row contributes
struct GpArgs {
    typedef E3Mul M;
    static constexpr int PLANE = 0;
    const u64 *a, *b;
    u64 *out;       // [3][N]
    e3 *totals;     // [nblocks]
    u64 g[3];
    u64 n;
    __device__ __forceinline__ e3 row(u64 i, e3 acc) const {
        running_put(*this, i, acc);
        const e3 num = e3_make(gl_add(a[i], g[0]), g[1], g[2]);
        const e3 den = e3_make(gl_add(b[i], g[0]), g[1], g[2]);
        return e3_mul(num, e3_inv(den));
    }
};
struct LuArgs {
    typedef E3Add M;
    static constexpr int PLANE = 6;
    const u64 *a, *t, *m;
    u64 *out;       // [9][N]
    e3 *totals;
    u64 n;
    u64 g[3];
    __device__ __forceinline__ e3 row(u64 i, e3 acc) const {
        const e3 h1 = e3_inv(e3_make(gl_add(a[i], g[0]), g[1], g[2]));
        const e3 h2 = e3_scale(e3_inv(e3_make(gl_add(t[i], g[0]), g[1], g[2])), m[i]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out[(u64)c * n + i] = h1.c[c];
            out[(u64)(3 + c) * n + i] = h2.c[c];
            out[(u64)(PLANE + c) * n + i] = acc.c[c];
        }
        return e3_sub(h1, h2);
    }
};

// the running values of the GP_PER rows from `base` on, each with `off` applied from the left
template <class Arg>
__device__ __forceinline__ void running_offset(const Arg &A, u64 base, e3 off) {
    for (int k = 0; k < GP_PER; k++) {
        const u64 i = base + k;
        if (i < A.n) running_put(A, i, Arg::M::op(off, running_get(A, i)));
    }
}

// inclusive Hillis-Steele scan of sh[GP_BLK], in place; the whole block calls it, its own sh[t] written and a barrier passed
template <class M>
__device__ __forceinline__ void block_scan(e3 *sh, int t) {
    for (int d = 1; d < GP_BLK; d <<= 1) {
        e3 v = sh[t];
        if (t >= d) v = M::op(sh[t - d], v);
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
}

template <class Arg>
__global__ void __launch_bounds__(GP_BLK) scan_local_kernel(Arg A) {
    typedef typename Arg::M M;
    __shared__ e3 sh[GP_BLK];
    const int t = threadIdx.x;
    const u64 base = ((u64)blockIdx.x * GP_BLK + t) * GP_PER;
    e3 acc = M::id();
    // exclusive scan inside the lane's run, stored without the lane / block prefix
    for (int k = 0; k < GP_PER; k++) {
        const u64 i = base + k;
        if (i < A.n) acc = M::op(acc, A.row(i, acc));
    }
    sh[t] = acc;
    __syncthreads();
    block_scan<M>(sh, t);
    const e3 lane_prefix = t ? sh[t - 1] : M::id();
    if (t == GP_BLK - 1) A.totals[blockIdx.x] = sh[t];
    running_offset(A, base, lane_prefix);
}

// exclusive scan of the block totals, in place, one workgroup (sequential over chunks of GP_BLK, the carry in LDS)
template <class M>
__global__ void __launch_bounds__(GP_BLK) scan_totals_kernel(e3 *totals, u64 nblocks) {
    __shared__ e3 sh[GP_BLK];
    __shared__ e3 carry;
    const int t = threadIdx.x;
    if (t == 0) carry = M::id();
    __syncthreads();
    for (u64 base = 0; base < nblocks; base += GP_BLK) {
        const u64 i = base + t;
        sh[t] = i < nblocks ? totals[i] : M::id();
        __syncthreads();
        block_scan<M>(sh, t);
        const e3 excl = M::op(carry, t ? sh[t - 1] : M::id());
        const e3 last = M::op(carry, sh[GP_BLK - 1]);
        __syncthreads();
        if (i < nblocks) totals[i] = excl;
        if (t == 0) carry = last;
        __syncthreads();
    }
}

template <class Arg>
__global__ void __launch_bounds__(GP_BLK) scan_apply_kernel(Arg A) {
    running_offset(A, ((u64)blockIdx.x * GP_BLK + threadIdx.x) * GP_PER, A.totals[blockIdx.x]);
}

// A: the input columns filled in by the entry point, which has checked its arguments
template <class Arg>
int32_t scan_launch(zp_ctx *ctx, Arg A, size_t n, const uint64_t gamma[3], uint64_t *d_out) {
    const u64 nblocks = (n + (u64)GP_BLK * GP_PER - 1) / ((u64)GP_BLK * GP_PER);
    u64 *scr = nullptr;
    ZP_TRY(zpi_scratch(ctx, 3, nblocks * 3 + 8, &scr));
    A.out = (u64 *)d_out; A.totals = (e3 *)scr; A.n = n;
    for (int i = 0; i < 3; i++) A.g[i] = gamma[i];
    hipLaunchKernelGGL(scan_local_kernel<Arg>, dim3((unsigned)nblocks), dim3(GP_BLK), 0, ctx->stream, A);
    hipLaunchKernelGGL(scan_totals_kernel<typename Arg::M>, dim3(1), dim3(GP_BLK), 0, ctx->stream, (e3 *)scr, nblocks);
    hipLaunchKernelGGL(scan_apply_kernel<Arg>, dim3((unsigned)nblocks), dim3(GP_BLK), 0, ctx->stream, A);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

}  // namespace

extern "C" int32_t zp_logup_columns(zp_ctx *ctx, const uint64_t *d_a, const uint64_t *d_t, const uint64_t *d_m, size_t n,
                                    const uint64_t gamma[3], uint64_t *d_out) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "logup_columns");
    ZP_ARG(ctx, n >= 1, "n must be >= 1");
    ZP_ARG(ctx, d_a && d_t && d_m && gamma && d_out, "null pointer");
    ZP_ARG(ctx, gamma[0] < GL_P && gamma[1] < GL_P && gamma[2] < GL_P, "challenge not canonical");
    LuArgs A;
    A.a = (const u64 *)d_a; A.t = (const u64 *)d_t; A.m = (const u64 *)d_m;
    return scan_launch(ctx, A, n, gamma, d_out);
}

extern "C" int32_t zp_grand_product(zp_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, size_t n, const uint64_t gamma[3],
                                    uint64_t *d_out) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "grand_product");
    ZP_ARG(ctx, n >= 1, "n must be >= 1");
    ZP_ARG(ctx, d_a && d_b && gamma && d_out, "null pointer");
    ZP_ARG(ctx, gamma[0] < GL_P && gamma[1] < GL_P && gamma[2] < GL_P, "challenge not canonical");
    GpArgs A;
    A.a = (const u64 *)d_a; A.b = (const u64 *)d_b;
    return scan_launch(ctx, A, n, gamma, d_out);
}

// ---- the walk over a program's stage-2 table (air_program.hpp: kinds, planes and input columns of an argument)
int32_t zpi_stage2_argument(zp_ctx *ctx, const u64 *st, const u64 *a, const u64 *b, const u64 *c, size_t N, const u64 g[3], u64 *d_s2, size_t *at) {
    uint64_t *out = (uint64_t *)(d_s2 + *at * N);
    *at += zpi_stage2_planes(st[0]);
    if (st[0] == ZPS2_PRODUCT) return zp_grand_product(ctx, (const uint64_t *)a, (const uint64_t *)b, N, (const uint64_t *)g, out);
    return zp_logup_columns(ctx, (const uint64_t *)a, (const uint64_t *)b, (const uint64_t *)c, N, (const uint64_t *)g, out);
}

int32_t zpi_stage2_columns(zp_ctx *ctx, const ZpProgram &pg, const u64 *d_trace, int logn, const u64 g[3], u64 *d_s2) {
    const size_t N = (size_t)1 << logn;
    size_t at = 0;
    for (size_t k = 0; k < pg.n_s2; k++) {
        const u64 *st = pg.stage2 + 4 * k;
        ZP_TRY(zpi_stage2_argument(ctx, st, d_trace + st[1] * N, d_trace + st[2] * N, d_trace + st[3] * N, N, g, d_s2, &at));
    }
    return ZP_OK;
}
