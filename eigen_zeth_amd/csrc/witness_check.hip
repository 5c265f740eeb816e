// zp_stark_check_witness on a ctx: the trace stays in HBM and is only read.  Entry point, refusals and the host path: csrc/witness_host.hip.
//   (1) witness_canonical_kernel: one streaming pass over all W * N words (the interpreter loads only the columns an instruction names), 16-byte
//       loads; a wave that saw a word >= p issues one atomicAdd on the count and one atomicMin on the first word index.
//   (2) the stage-2 columns by the prover's own primitives (zp_grand_product / zp_logup_columns) and one period of every sparse fixed column
//       (zpi_fixed_periods_build: the first half of the prover's fixed-column build, no transform -- on the trace domain a period IS the column).
//   (3) witness_program_kernel: quotient_program_kernel's shape (csrc/stark.hip: lane = row, slot file in LDS as [slot][lane], the instruction
//       word wave-uniform, every operand kind a uniform branch) on the TRACE domain.  The loop is written out here over air_program.hpp's field
//       accessors and constants, NOT as an environment of zpi_program_walk: as one it measured 1 % slower on the MI355X with the same vector
//       and LDS instructions (profiles/program_walk_static_and_ab.txt).  Next row = r + 1 mod N, the selectors
//       computed from r, x = w^r from the plan's two-level table; at an OUT no accumulation but a ballot of the lanes whose value is not 0 --
//       only when it is not empty one lane adds its popcount to the constraint's count and lowers the constraint's first row and the call's
//       first (row, constraint) key.  An honest trace issues no atomic at all.
// (2) and (3) run only when (1) found nothing: the field code takes canonical words.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "witness_merge.hpp"

namespace {

typedef unsigned long long ull;

__device__ __forceinline__ ull wave_min_u64(ull v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const ull t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ ull wave_add_u64(ull v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// words [head, head + 2 npairs) as 16-byte pairs (p + head is 16-byte aligned), grid-stride; the word in front of them (head = 1) and the one
// behind them (an odd rest) are lane 0's.  res[0] += words >= p, res[1] = min(res[1], index of such a word)
__global__ void __launch_bounds__(256) witness_canonical_kernel(const u64 *__restrict__ p, u64 total, u64 head, u64 npairs, ull *res) {
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, stride = (u64)gridDim.x * 256;
    const ulonglong2 *q = (const ulonglong2 *)(p + head);
    ull cnt = 0, mn = ~0ULL;
#pragma unroll 4
    for (u64 i = tid; i < npairs; i += stride) {
        const ulonglong2 v = q[i];
        const u64 at = head + 2 * i;
        if (v.y >= GL_P) { cnt++; mn = at + 1 < mn ? at + 1 : mn; }
        if (v.x >= GL_P) { cnt++; mn = at < mn ? at : mn; }
    }
    if (tid == 0) {
        const u64 tail = head + 2 * npairs;
        if (tail < total && p[tail] >= GL_P) { cnt++; mn = tail < mn ? tail : mn; }
        if (head && p[0] >= GL_P) { cnt++; mn = 0; }
    }
    if (__ballot(cnt != 0) == 0) return;                 // wave-uniform
    const ull c = wave_add_u64(cnt), m = wave_min_u64(mn);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&res[0], c);
        atomicMin(&res[1], m);
    }
}

struct WProgArgs {
    const u64 *prog;            // device copy of header | constants | instructions
    const u64 *trace, *s2;      // columns idx < W: the caller's trace (read only); the rest: the stage-2 scratch
    const u64 *pub;             // publics, then the challenge
    const u64 *xs_lo, *xs_hi;   // w_N^e = lo[e & (2^lb - 1)] * hi[e >> lb]
    const u64 *fixedx, *fx_tab; // one period per sparse column; (offset, index mask) per column
    ull *counts, *first_row, *first_key;
    u64 N, wlast;
    u64 stride, row0, nrows;    // the row-window form only: trace columns [W][stride], rows [row0, row0 + nrows) of the domain
    int W, lb, n_const, n_instr;
};

// WINDOW = false: the whole trace domain.  WINDOW = true: rows [row0, row0 + nrows) of it, what one rank of a sharded proof judges
// (zpi_witness_sharded) -- a trace column is [stride] words, row r at r - row0, and unless nrows == N ONE halo row at index nrows holds row
// (row0 + nrows) mod N, the next rank's first.  The stage-2 columns stay whole, [W2][N], read at the global row and the global next row; the
// selectors, the sparse periods, x and every reported row are the GLOBAL row's.  A dead lane walks the window's first row.
template <bool WINDOW>
__global__ void __launch_bounds__(256) witness_program_kernel(WProgArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 slots[];   // [n_slots][256]
    const int tid = threadIdx.x;
    const u64 wi = (u64)blockIdx.x * 256 + tid;                   // the row inside the window (the whole domain: the row)
    const bool live = wi < (WINDOW ? a.nrows : a.N);
    const u64 ii = live ? wi : 0;                                 // a dead lane walks the first row: in bounds, masked out of every ballot
    const u64 r = WINDOW ? a.row0 + wi : wi, rr = WINDOW ? a.row0 + ii : ii;
    const u64 rn = (rr + 1) & (a.N - 1);
    const u64 st = WINDOW ? a.stride : a.N;                       // a trace column's words, where its row and its next row sit
    const u64 tc = WINDOW ? ii : rr, tn = WINDOW ? (a.nrows == a.N ? rn : ii + 1) : rn;
    const u64 x = gl_mul(a.xs_lo[rr & ((1ULL << a.lb) - 1)], a.xs_hi[rr >> a.lb]);
    const u64 xml = gl_sub(x, a.wlast);
    const u64 *consts = a.prog + ZPH_WORDS, *ins = consts + a.n_const;
    int k_out = 0;
    for (int i = 0; i < a.n_instr; i++) {
        const u64 wu = zpi_wave_uniform(ins[i]);                  // uniform address: scalar load
        const int op = zpi_op(wu), dst = zpi_dst(wu);
        u64 v[2];
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int kind = zpi_kind(wu, o), idx = zpi_idx(wu, o);
            u64 val;
            switch (kind) {
                case ZPK_SLOT: val = slots[idx * 256 + tid]; break;
                case ZPK_COL: val = idx < a.W ? a.trace[(u64)idx * st + tc] : a.s2[(u64)(idx - a.W) * a.N + rr]; break;
                case ZPK_NEXT: val = idx < a.W ? a.trace[(u64)idx * st + tn] : a.s2[(u64)(idx - a.W) * a.N + rn]; break;
                case ZPK_FIXED:
                    if (idx == 0) val = rr == 0;
                    else if (idx == 1) val = rr == a.N - 1;
                    else val = a.fixedx[a.fx_tab[2 * (idx - 2)] + (rr & a.fx_tab[2 * (idx - 2) + 1])];
                    break;
                case ZPK_PUB: val = a.pub[idx]; break;
                case ZPK_CONST: val = consts[idx]; break;
                default: val = xml; break;
            }
            v[o] = val;
            if (op == ZPI_OUT) break;
        }
        if (op == ZPI_ADD) slots[dst * 256 + tid] = gl_add(v[0], v[1]);
        else if (op == ZPI_SUB) slots[dst * 256 + tid] = gl_sub(v[0], v[1]);
        else if (op == ZPI_MUL) slots[dst * 256 + tid] = gl_mul(v[0], v[1]);
        else {
            const ull m = __ballot(live && v[0] != 0);            // wave-uniform
            if (m != 0 && (tid & 63) == __ffsll((long long)m) - 1) {      // the lowest violating lane of the wave: its row is the wave's smallest
                atomicAdd(&a.counts[k_out], (ull)__popcll(m));
                atomicMin(&a.first_row[k_out], (ull)r);
                atomicMin(a.first_key, ((ull)r << 24) | (ull)k_out);
            }
            k_out++;
        }
    }
}

}  // namespace

// (1) the canonical pass over W * 2^logn words: *bad_n = words >= p, *bad_at = the index of the first in memory order (~0: none).  Synchronised.
int32_t zpi_witness_canonical(zp_ctx *ctx, const u64 *d_trace, size_t total, u64 *bad_n, u64 *bad_at) {
    ZP_ARG(ctx, (uintptr_t)d_trace % 8 == 0, "trace pointer not aligned");
    void *poolv = nullptr;
    ZP_TRY(zpi_pool_alloc(ctx, 16, &poolv));
    struct Release { zp_ctx *c; void *p; ~Release() { zpi_pool_release(c, p, 16); } } release_{ctx, poolv};
    ull *res = (ull *)poolv;
    ZpStage stage_(ctx, "witness_canonical");
    ZP_HIP(ctx, hipMemsetAsync(res, 0, 8, ctx->stream));
    ZP_HIP(ctx, hipMemsetAsync(res + 1, 0xFF, 8, ctx->stream));
    const u64 head = ((uintptr_t)d_trace % 16) ? 1 : 0, npairs = (total - head) / 2;
    u64 blocks = (npairs + 255) / 256, cap = (u64)ctx->num_cu * 8;
    blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
    hipLaunchKernelGGL(witness_canonical_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_trace, (u64)total, head, npairs, res);
    ZP_HIP(ctx, hipGetLastError());
    u64 out[2];
    ZP_TRY(zpi_d2h_small(ctx, out, res, 16));
    *bad_n = out[0]; *bad_at = out[1];
    return ZP_OK;
}

// the report of a trace with words >= p: the constraints are not evaluated
void zpi_witness_noncanonical_report(size_t K, size_t N, u64 bad_n, u64 bad_at, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row) {
    const u64 rep[8] = {ZP_WITNESS_NONCANONICAL, ~0ULL, ~0ULL, 0, 0, bad_n, bad_at / N, bad_at % N};
    memcpy(h_report, rep, sizeof rep);
    if (h_counts) memset(h_counts, 0, K * 8);
    if (h_first_row) memset(h_first_row, 0xFF, K * 8);
}

// (3) the constraints over (trace, GIVEN stage-2 columns on the trace domain, publics then the challenge): one period of every sparse fixed column,
// then either the generated kernel of this program (AIR plug-in ABI: `<symbol>_witness`, registered under the digest dg32 by
// zp_stark_set_air_kernel_witness; knob "witness_kernel" = 1; stage "witness_program_gen") with [publics | challenge | 0] as its only upload, or
// the interpreter over the uploaded program (stage "witness_program").  One result buffer [first key][first_row: K][counts: K].
// win = NULL: the whole domain, d_trace u64[W][N].  Else rows [win->row0, win->row0 + win->nrows) of it, d_trace u64[W][win->stride] with the halo
// row (witness_program_kernel<true>); the kernel is `<symbol>_witness_rows` (zp_stark_set_air_kernel_witness_rows), the stages
// "witness_program_rows_gen" / "witness_program_rows".  d_s2 is whole either way.  pubchal: publics, then the challenge when the program has
// stage-2 arguments (a trailing pad word is ignored); dg32 = NULL: no kernel is looked up.  The result stays on the device: d_res, 1 + 2 K words.
int32_t zpi_witness_launch(zp_ctx *ctx, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace, const u64 *d_s2,
                           int logn, const ZpWitnessWindow *win, u64 *d_res) {
    ZP_BIND(ctx);
    ZP_ARG(ctx, logn >= 1 && logn <= 30, "logn out of range");
    for (const ZpFixedCol &fc : pg.fxc) ZP_ARG(ctx, fc.lp <= logn, "fixed column longer than the trace");
    const size_t N = (size_t)1 << logn, K = pg.K, n_pc = pg.n_pub + pg.n_chal;
    ZP_ARG(ctx, pubchal.size() >= n_pc, "publics and challenge shorter than the program's");
    if (win)      // every index the window form computes stays inside [W][stride]: rows, and the halo unless the window is the domain
        ZP_ARG(ctx, win->nrows >= 1 && win->row0 + win->nrows <= N && win->stride >= win->nrows + (win->nrows == N ? 0 : 1), "row window outside the trace domain");
    NttPlan *pl;
    ZP_TRY(zpi_get_plan(ctx, logn, false, &pl));
    void *plug = nullptr;
    if (dg32 && ctx->tune_witness_kernel) {
        auto it = ctx->air_kernels.find(zpi_air_kernel_key(win ? "witness_rows:" : "witness:", dg32));
        if (it != ctx->air_kernels.end()) plug = it->second;
    }
    ull *res = (ull *)d_res;
    ZpStage stage_(ctx, win ? (plug ? "witness_program_rows_gen" : "witness_program_rows") : (plug ? "witness_program_gen" : "witness_program"));
    ZP_HIP(ctx, hipMemsetAsync(res, 0xFF, (1 + K) * 8, ctx->stream));
    ZP_HIP(ctx, hipMemsetAsync(res + 1 + K, 0, K * 8, ctx->stream));
    u64 *d_periods = nullptr;
    size_t period_words = 0;
    ZP_TRY(zpi_fixed_periods_build(ctx, pg.words, pg.fxc, (const uint64_t *)pubchal.data(), 0, false, &d_periods, &period_words));
    const u64 wlast = gl_inv(gl_root(ctx->root32, logn));
    const size_t rows = win ? win->nrows : N;
    if (plug) {
        std::vector<u64> ops(pubchal.begin(), pubchal.begin() + n_pc);
        ops.push_back(0);                         // never empty
        u64 *d_ops;
        ZP_TRY(zpi_scratch(ctx, 3, ops.size(), &d_ops));
        ZP_TRY(zpi_h2d(ctx, d_ops, ops.data(), ops.size() * 8));
        const uint64_t *s2 = (const uint64_t *)(d_s2 ? d_s2 : d_trace), *periods = (const uint64_t *)(d_periods ? d_periods : d_ops);
        const int hrc = win ? ((zp_air_witness_rows_fn)plug)((void *)ctx->stream, (const uint64_t *)d_trace, (uint64_t)win->stride, s2, periods, (const uint64_t *)d_ops,
                                                            (const uint64_t *)pl->d_twl, (const uint64_t *)pl->d_twh, pl->lb, (uint64_t)N, (uint64_t)win->row0,
                                                            (uint64_t)win->nrows, wlast, (uint64_t *)res)
                            : ((zp_air_witness_fn)plug)((void *)ctx->stream, (const uint64_t *)d_trace, s2, periods, (const uint64_t *)d_ops, (const uint64_t *)pl->d_twl,
                                                       (const uint64_t *)pl->d_twh, pl->lb, (uint64_t)N, wlast, (uint64_t *)res);
        if (hrc != 0) {
            ctx->err = "generated witness kernel: launch failed (hip error " + std::to_string(hrc) + ")";
            return ZP_ERR_HIP;
        }
    } else {
        // the upload comes after whatever made the stage-2 columns: those primitives use the same scratch slot
        ZpProgramDev dv;
        ZP_TRY(zpi_program_upload(ctx, pg, ZpSpan{pubchal.data(), n_pc}, {}, 0, &dv));
        WProgArgs a;
        a.prog = dv.consts - ZPH_WORDS; a.trace = d_trace; a.s2 = d_s2 ? d_s2 : d_trace; a.pub = dv.pubchal; a.fx_tab = dv.fx_tab; a.fixedx = d_periods;
        a.xs_lo = pl->d_twl; a.xs_hi = pl->d_twh; a.lb = pl->lb;
        a.first_key = res; a.first_row = res + 1; a.counts = res + 1 + K;
        a.N = N; a.wlast = wlast;
        a.stride = win ? win->stride : N; a.row0 = win ? win->row0 : 0; a.nrows = rows;
        a.W = (int)pg.W; a.n_const = (int)pg.n_const; a.n_instr = (int)pg.n_instr;
        const dim3 grid((unsigned)((rows + 255) / 256));
        if (win) hipLaunchKernelGGL(witness_program_kernel<true>, grid, dim3(256), pg.slot_file() * 256 * 8, ctx->stream, a);
        else hipLaunchKernelGGL(witness_program_kernel<false>, grid, dim3(256), pg.slot_file() * 256 * 8, ctx->stream, a);
        ZP_HIP(ctx, hipGetLastError());
    }
    return ZP_OK;
}

// ... over the whole domain, with the report.  Both single-GPU callers -- zp_stark_check_witness on a ctx and the one-call provers under
// "prove_check" -- come through here.
int32_t zpi_witness_constraints(zp_ctx *ctx, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace, const u64 *d_s2,
                                int logn, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row) {
    const size_t res_words = zpi_witness_result_words(pg.K);
    void *poolv = nullptr;
    ZP_TRY(zpi_pool_alloc(ctx, res_words * 8, &poolv));
    struct Release { zp_ctx *c; void *p; size_t b; ~Release() { zpi_pool_release(c, p, b); } } release_{ctx, poolv, res_words * 8};
    std::vector<u64> out(res_words);
    ZP_TRY(zpi_witness_launch(ctx, pg, dg32, pubchal, d_trace, d_s2, logn, nullptr, (u64 *)poolv));
    ZP_TRY(zpi_d2h(ctx, out.data(), poolv, res_words * 8));
    zpi_witness_report((const uint64_t *)out.data(), pg.K, h_report, h_counts, h_first_row);
    return ZP_OK;
}

// zp_stark_check_witness on a ctx: (1), then (2) the stage-2 columns made HERE from the trace at the caller's challenge, then (3)
int32_t zpi_witness_check_device(zp_ctx *ctx, const ZpProgram &pg, const std::vector<u64> &pubchal, const u64 *d_trace, int logn, uint64_t *h_report,
                                 uint64_t *h_counts, uint64_t *h_first_row) {
    ZP_BIND(ctx);
    ZP_ARG(ctx, logn <= 30, "logn out of range");
    const size_t N = (size_t)1 << logn;
    u64 bad_n, bad_at;
    ZP_TRY(zpi_witness_canonical(ctx, d_trace, pg.W * N, &bad_n, &bad_at));
    if (bad_n != 0) {
        zpi_witness_noncanonical_report(pg.K, N, bad_n, bad_at, h_report, h_counts, h_first_row);
        return ZP_OK;
    }
    const size_t s2_bytes = (pg.W2 * N ? pg.W2 * N : 1) * 8;
    void *s2v = nullptr;
    ZP_TRY(zpi_pool_alloc(ctx, s2_bytes, &s2v));
    struct Release { zp_ctx *c; void *p; size_t b; ~Release() { zpi_pool_release(c, p, b); } } release_{ctx, s2v, s2_bytes};
    u64 *s2 = (u64 *)s2v;
    {
        ZpStage stage_(ctx, "witness_stage2");
        ZP_TRY(zpi_stage2_columns(ctx, pg, d_trace, logn, pubchal.data() + pg.n_pub, s2));
    }
    // the digest names the kernel: one SHA-256 of the blob per call (a program of >= 2^14 words: one memcmp against the ctx's digest cache) -- paid only
    // by a ctx that has a generated kernel registered and the knob on; the provers pass the digest their transcript needs anyway
    uint8_t dg[32];
    const bool lookup = ctx->tune_witness_kernel && !ctx->air_kernels.empty();
    if (lookup) zpi_program_digest_cached(ctx, pg.words, pg.n_words, dg);
    return zpi_witness_constraints(ctx, pg, lookup ? dg : nullptr, pubchal, d_trace, s2, logn, h_report, h_counts, h_first_row);
}
