// zp_stark_diagnose_stage2 on a ctx: a hash join in HBM.  Entry point, refusals, the host path and what the records mean: csrc/stage2_diag_host.hip.
//   (0) the canonical pass of the witness check (zpi_witness_canonical): the table's empty key is ~0, which no canonical word is.
//   Then per argument of the stage-2 table, on ONE table that is reset in between:
//   (1) s2_insert_kernel, lane = row: the slot of a[r] is found or claimed by atomicCAS on the key with linear probing -- the value the CAS returns
//       is the ONLY view of a key this kernel takes (a plain load may be served by another XCD's stale L2 inside a launch) --, then atomicAdd on lhs
//       and atomicMin on first_a; the same for b[r] (t[r]) with rhs += 1 (m[r]) and first_b.  rhs is a 128-bit integer sum (rhs_lo, rhs_hi: the
//       carry comes from the value the atomicAdd on rhs_lo returns), reduced mod p by its readers.  The probe loop is bounded by the capacity; a
//       lane that exhausts it raises the error flag (ZP_ERR_INTERNAL) -- with capacity >= 4 N and at most 2 N keys that is a bug, not a load.  No
//       lane waits for another.  A wave whose live lanes all carry one key ("s2_diag_merge", default on) sends one lane: a whole column of one
//       value is N / 64 atomics per word instead of N on one address.
//   (2) s2_compare_kernel, lane = slot (a launch of its own: plain loads): a slot whose lhs != rhs mod p is unbalanced; ballot, then the wave's first
//       such lane adds the wave's count and its sum of lhs and lowers r_a / r_b by the wave's minima.  An honest trace issues no atomic.
//   (3) s2_record_kernel: probes the slots of a[r_a] and b[r_b] and writes the argument's record.
// All records come down in one copy at the end.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"

namespace {

typedef unsigned long long ull;
constexpr ull EMPTY = ~0ULL;

// struct of arrays, each [cap]: key | lhs | rhs_lo | rhs_hi | first_a | first_b
struct S2Table {
    ull *key, *lhs, *rhs_lo, *rhs_hi, *first_a, *first_b;
    u64 mask;       // cap - 1, cap a power of two
    int shift;      // 64 - log2(cap)
};

// multiply-shift over the folded word: the top bits of the product depend on every bit of v
__device__ __forceinline__ u64 s2_hash(u64 v, int shift) { return ((v ^ (v >> 32)) * 0x9E3779B97F4A7C15ULL) >> shift; }
// (hi, lo) as an integer below 2^96, mod p: 2^64 = 2^32 - 1 (mod p)
__device__ __forceinline__ u64 s2_reduce(u64 lo, u64 hi) { return gl_add(lo >= GL_P ? lo - GL_P : lo, hi * 0xFFFFFFFFULL); }

__device__ __forceinline__ ull wave_min(ull v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const ull t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ ull wave_sum(ull v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ ull wave_sum_mod(ull v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = gl_add(v, (u64)__shfl_xor(v, o));
    return v;
}

// the slot that holds v, claimed if nobody had: decided by what atomicCAS returns alone.  ~0: the probe went round the whole table
__device__ __forceinline__ u64 s2_claim(const S2Table &t, u64 v) {
    u64 s = s2_hash(v, t.shift);
    for (u64 trip = 0; trip <= t.mask; trip++, s = (s + 1) & t.mask) {
        const ull old = atomicCAS(&t.key[s], EMPTY, (ull)v);
        if (old == EMPTY || old == (ull)v) return s;
    }
    return EMPTY;
}
// ... found with plain loads, in a later launch.  ~0: not there
__device__ __forceinline__ u64 s2_find(const S2Table &t, u64 v) {
    u64 s = s2_hash(v, t.shift);
    for (u64 trip = 0; trip <= t.mask; trip++, s = (s + 1) & t.mask) {
        const ull k = t.key[s];
        if (k == (ull)v) return s;
        if (k == EMPTY) break;
    }
    return EMPTY;
}

// one side of one row: value v at row r with weight w (1, or m[r] on the table side of a lookup: MODSUM).  A dead lane carries w = 0 and r = ~0.
template <bool MERGE, bool BSIDE, bool MODSUM>
__device__ __forceinline__ void s2_tally(const S2Table &t, bool live, u64 v, u64 r, u64 w, unsigned *err) {
    bool mine = live;
    if (MERGE) {
        const ull act = __ballot(live);                           // wave-uniform
        if (act == 0) return;
        const int lead = __ffsll((long long)act) - 1;
        const u64 v0 = (u64)__shfl((ull)v, lead);
        if (__ballot(live && v == v0) == act && (act & (act - 1)) != 0) {      // one key, more than one lane
            r = wave_min(r);
            w = MODSUM ? wave_sum_mod(w) : wave_sum(w);
            mine = (int)(threadIdx.x & 63) == lead;
        }
    }
    if (!mine) return;
    const u64 s = s2_claim(t, v);
    if (s == EMPTY) { atomicOr(err, 1u); return; }
    if (!BSIDE) {
        atomicAdd(&t.lhs[s], (ull)w);
        atomicMin(&t.first_a[s], (ull)r);
    } else {
        const ull old = atomicAdd(&t.rhs_lo[s], (ull)w);
        if (old + w < old) atomicAdd(&t.rhs_hi[s], 1ULL);
        atomicMin(&t.first_b[s], (ull)r);
    }
}

// m = NULL: a permutation {a, b}; else a lookup {a, b = t, m}
template <bool MERGE>
__global__ void __launch_bounds__(256) s2_insert_kernel(S2Table t, const u64 *__restrict__ a, const u64 *__restrict__ b, const u64 *__restrict__ m, u64 N,
                                                        unsigned *err) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool live = r < N;
    const u64 row = live ? r : EMPTY;
    s2_tally<MERGE, false, false>(t, live, live ? a[r] : 0, row, live ? 1 : 0, err);
    if (m) s2_tally<MERGE, true, true>(t, live, live ? b[r] : 0, row, live ? m[r] : 0, err);
    else s2_tally<MERGE, true, false>(t, live, live ? b[r] : 0, row, live ? 1 : 0, err);
}

// res[0] += unbalanced slots, res[1] += their lhs, res[2] = min first_a, res[3] = min first_b over them
__global__ void __launch_bounds__(256) s2_compare_kernel(S2Table t, ull *res) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;            // the grid is cap / 256 blocks, or one block of cap lanes
    const bool live = s <= t.mask;
    ull lhs = 0, fa = EMPTY, fb = EMPTY;
    bool bad = false;
    if (live && t.key[s] != EMPTY) {
        lhs = t.lhs[s];
        bad = lhs != s2_reduce(t.rhs_lo[s], t.rhs_hi[s]);
        if (bad) { fa = t.first_a[s]; fb = t.first_b[s]; }
    }
    const ull mk = __ballot(bad);                                 // wave-uniform
    if (mk == 0) return;
    const ull sum = wave_sum(bad ? lhs : 0), ma = wave_min(fa), mb = wave_min(fb);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mk) - 1) {
        atomicAdd(&res[0], (ull)__popcll(mk));
        atomicAdd(&res[1], sum);
        atomicMin(&res[2], ma);
        atomicMin(&res[3], mb);
    }
}

// lane 0: words 0, 1, 2, 11 and the a side (3..6); lane 1: the b side (7..10)
__global__ void __launch_bounds__(64) s2_record_kernel(S2Table t, const u64 *__restrict__ a, const u64 *__restrict__ b, const ull *res, u64 kind, u64 *rec,
                                                       unsigned *err) {
    const int side = threadIdx.x;
    if (side > 1) return;
    const u64 row = res[2 + side];
    u64 v = EMPTY, lhs = 0, rhs = 0;
    if (row != EMPTY) {
        v = (side ? b : a)[row];
        const u64 s = s2_find(t, v);
        if (s == EMPTY) atomicOr(err, 2u);
        else { lhs = t.lhs[s]; rhs = s2_reduce(t.rhs_lo[s], t.rhs_hi[s]); }
    }
    u64 *o = rec + 3 + 4 * side;
    o[0] = row; o[1] = v; o[2] = lhs; o[3] = rhs;
    if (side == 0) {
        rec[0] = res[0] ? ZP_S2_FAILS : ZP_S2_HOLDS;
        rec[1] = kind;
        rec[2] = res[0];
        rec[11] = res[1];
    }
}

}  // namespace

int32_t zpi_stage2_diag_device(zp_ctx *ctx, const ZpProgram &pg, const u64 *d_trace, int logn, uint64_t *h_diag) {
    ZP_BIND(ctx);
    ZP_ARG(ctx, logn <= 30, "logn out of range");
    const size_t N = (size_t)1 << logn, n_s2 = pg.n_s2;
    u64 bad_n, bad_at;
    ZP_TRY(zpi_witness_canonical(ctx, d_trace, pg.W * N, &bad_n, &bad_at));
    if (bad_n != 0) {
        zpi_stage2_diag_noncanonical(pg, h_diag);
        return ZP_OK;
    }
    const int logcap = logn + 2;                                  // the smallest power of two >= 4 N: at most 2 N keys, load <= 1/2
    const size_t cap = (size_t)1 << logcap;
    // [table: 6 cap][per argument: res 4][records: ZP_S2_WORDS each][error flag]
    const size_t small_words = n_s2 * (4 + ZP_S2_WORDS) + 1, bytes = (6 * cap + small_words) * 8;
    void *poolv = nullptr;
    ZP_TRY(zpi_pool_alloc(ctx, bytes, &poolv));
    struct Release { zp_ctx *c; void *p; size_t b; ~Release() { zpi_pool_release(c, p, b); } } release_{ctx, poolv, bytes};
    ull *base = (ull *)poolv;
    S2Table t;
    t.key = base; t.lhs = base + cap; t.rhs_lo = base + 2 * cap; t.rhs_hi = base + 3 * cap; t.first_a = base + 4 * cap; t.first_b = base + 5 * cap;
    t.mask = cap - 1; t.shift = 64 - logcap;
    ull *res = base + 6 * cap;
    u64 *rec = (u64 *)(res + 4 * n_s2);
    unsigned *err = (unsigned *)(rec + n_s2 * ZP_S2_WORDS);
    ZpStage stage_(ctx, "stage2_diagnose");
    ZP_HIP(ctx, hipMemsetAsync(res, 0, small_words * 8, ctx->stream));
    for (size_t j = 0; j < n_s2; j++) ZP_HIP(ctx, hipMemsetAsync(res + 4 * j + 2, 0xFF, 16, ctx->stream));
    const dim3 rows_grid((unsigned)((N + 255) / 256)), slots_grid((unsigned)((cap + 255) / 256));
    for (size_t j = 0; j < n_s2; j++) {
        const u64 *st = pg.stage2 + 4 * j;
        const u64 *a = d_trace + st[1] * N, *b = d_trace + st[2] * N, *m = st[0] == ZPS2_LOGUP ? d_trace + st[3] * N : nullptr;
        ZP_HIP(ctx, hipMemsetAsync(t.key, 0xFF, cap * 8, ctx->stream));
        ZP_HIP(ctx, hipMemsetAsync(t.lhs, 0, 3 * cap * 8, ctx->stream));
        ZP_HIP(ctx, hipMemsetAsync(t.first_a, 0xFF, 2 * cap * 8, ctx->stream));
        if (ctx->tune_s2_diag_merge) hipLaunchKernelGGL(s2_insert_kernel<true>, rows_grid, dim3(256), 0, ctx->stream, t, a, b, m, (u64)N, err);
        else hipLaunchKernelGGL(s2_insert_kernel<false>, rows_grid, dim3(256), 0, ctx->stream, t, a, b, m, (u64)N, err);
        ZP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(s2_compare_kernel, slots_grid, dim3(256), 0, ctx->stream, t, res + 4 * j);
        ZP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(s2_record_kernel, dim3(1), dim3(64), 0, ctx->stream, t, a, b, (const ull *)(res + 4 * j), st[0], rec + j * ZP_S2_WORDS, err);
        ZP_HIP(ctx, hipGetLastError());
    }
    std::vector<u64> down(n_s2 * ZP_S2_WORDS + 1);
    ZP_TRY(zpi_d2h(ctx, down.data(), rec, down.size() * 8));
    if ((unsigned)down.back() != 0) {
        ctx->err = "stage-2 diagnosis: the hash table's probe bound was exhausted";
        return ZP_ERR_INTERNAL;
    }
    memcpy(h_diag, down.data(), n_s2 * ZP_S2_WORDS * 8);
    return ZP_OK;
}
