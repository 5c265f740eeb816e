// What is not the transform but streams u64 matrices: the HBM copy probe, and the layout kernels of the multi-GPU paths.
#include "ctx.hpp"

#define ZP_LDG(p) __builtin_nontemporal_load(p)
#define ZP_STG(p, v) __builtin_nontemporal_store(v, p)

// ---- measurement: what this device sustains on a plain copy, with this library's own kernel (16 bytes per lane, one persistent workgroup
// per CU by default since round 5) -- the ceiling bench.py prints next to the vendor peak
typedef __attribute__((ext_vector_type(4))) unsigned int zp_u32x4;
// U loads of 16 bytes in flight per lane, then U stores; NT: non-temporal policy (the data is touched once) or the default one.  Which grid,
// block size, depth and policy stream fastest is MEASURED (tools/ntt_r5_ab.py -> profiles/r5_ntt_ab.txt; knobs copy_grid / copy_block /
// copy_unroll / copy_nt): round 5 found one workgroup per CU (256 x 256 lanes, 4 in flight) at 5.6 TB/s against 4.9 for the 2048-workgroup
// grid of rounds 1-4 -- fewer concurrent streams, not more, is what HBM3E wants.
template <int U, bool NT>
__global__ void __launch_bounds__(1024) hbm_copy_kernel(const zp_u32x4 *__restrict__ in, zp_u32x4 *__restrict__ out, size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (U - 1) * stride < n16; i += U * stride) {
        zp_u32x4 v[U];
#pragma unroll
        for (int k = 0; k < U; k++) v[k] = NT ? __builtin_nontemporal_load(in + i + k * stride) : in[i + k * stride];
#pragma unroll
        for (int k = 0; k < U; k++) {
            if (NT) __builtin_nontemporal_store(v[k], out + i + k * stride);
            else out[i + k * stride] = v[k];
        }
    }
    for (; i < n16; i += stride) out[i] = in[i];
}

extern "C" int32_t zp_hbm_copy_probe(zp_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, int32_t reps, float *ms_per_copy) {
    if (!ctx) return ZP_ERR_ARG;
    ZP_BIND(ctx);
    ZP_ARG(ctx, d_src && d_dst && ms_per_copy && reps >= 1 && (bytes & 15) == 0 && bytes >= 16, "bad arguments");
    hipEvent_t e0, e1;
    ZP_HIP(ctx, hipEventCreate(&e0));
    ZP_HIP(ctx, hipEventCreate(&e1));
    const unsigned grid = ctx->tune_copy_grid > 0 ? (unsigned)ctx->tune_copy_grid : 256u;
    const unsigned block = (ctx->tune_copy_block == 512 || ctx->tune_copy_block == 1024) ? (unsigned)ctx->tune_copy_block : 256u;
    const bool u8 = ctx->tune_copy_unroll == 8;
    auto k = ctx->tune_copy_nt ? (u8 ? hbm_copy_kernel<8, true> : hbm_copy_kernel<4, true>) : (u8 ? hbm_copy_kernel<8, false> : hbm_copy_kernel<4, false>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, ctx->stream, (const zp_u32x4 *)d_src, (zp_u32x4 *)d_dst, bytes / 16);
    ZP_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; r++)
        hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, ctx->stream, (const zp_u32x4 *)d_src, (zp_u32x4 *)d_dst, bytes / 16);
    ZP_HIP(ctx, hipEventRecord(e1, ctx->stream));
    ZP_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    ZP_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_copy = ms / reps;
    return ZP_OK;
}

// ---- layout kernels of the multi-GPU paths: the send-buffer packing of the column->row all-to-all and the
// local transposes of the four-step NTT.  (Round 1 did these with generic tensor copies: 21 G elements/s for a four-step
// transform on one GPU against 75 G for the plain one.)
// out[h][w][j] = in[w][h*Mg + j]:  [Wl][G*Mg] -> [G][Wl][Mg]; runs of Mg contiguous elements, 16 bytes per lane
__global__ void __launch_bounds__(256) pack_blocks_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u64 Wl, u64 G, u64 Mg) {
    const u64 total2 = Wl * G * Mg / 2;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total2; i += (u64)gridDim.x * 256) {
        const u64 e = 2 * i, j = e % Mg, w = (e / Mg) % Wl, h = e / (Mg * Wl);
        const u64 *src = in + w * (G * Mg) + h * Mg + j;
        u64 *dst = out + e;
        dst[0] = ZP_LDG(src);
        dst[1] = ZP_LDG(src + 1);
    }
}
// out[c][r] = in[r][c], 64 x 64 tiles through LDS (row length 65: the column reads of the write phase hit 64 banks)
__global__ void __launch_bounds__(256) transpose_u64_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u64 R, u64 C) {
    __shared__ u64 tile[64][65];
    const u64 tiles_c = (C + 63) / 64;
    const u64 r0 = (blockIdx.x / tiles_c) * 64, c0 = (blockIdx.x % tiles_c) * 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const u64 r = r0 + i * 4 + w, c = c0 + lane;
        if (r < R && c < C) tile[i * 4 + w][lane] = ZP_LDG(&in[r * C + c]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const u64 c = c0 + i * 4 + w, r = r0 + lane;
        if (r < R && c < C) ZP_STG(&out[c * R + r], tile[lane][i * 4 + w]);
    }
}

extern "C" int32_t zp_pack_blocks(zp_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, size_t rows, size_t row_len, int32_t parts) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "pack_blocks");
    ZP_ARG(ctx, d_in && d_out && d_in != d_out && parts >= 1 && row_len % (size_t)parts == 0, "bad arguments");
    const size_t Mg = row_len / parts;
    ZP_ARG(ctx, Mg % 2 == 0 || rows * row_len == 0, "part length must be even");
    if (rows * row_len == 0) return ZP_OK;
    const size_t total2 = rows * row_len / 2;
    const unsigned blocks = (unsigned)(total2 / 256 + 1 < 8192 ? total2 / 256 + 1 : 8192);
    hipLaunchKernelGGL(pack_blocks_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const u64 *)d_in, (u64 *)d_out, (u64)rows, (u64)parts, (u64)Mg);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

extern "C" int32_t zp_transpose(zp_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, size_t rows, size_t cols) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "transpose");
    ZP_ARG(ctx, d_in && d_out && d_in != d_out, "bad arguments");
    if (rows * cols == 0) return ZP_OK;
    const size_t tiles = ((rows + 63) / 64) * ((cols + 63) / 64);
    ZP_ARG(ctx, tiles < (1ULL << 31), "matrix too large for one launch");
    hipLaunchKernelGGL(transpose_u64_kernel, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, (const u64 *)d_in, (u64 *)d_out, (u64)rows, (u64)cols);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}
