// BN254 (alt_bn128) G1 multi-scalar multiplication: sum_i s_i * P_i   (SURVEY.md 8a N6).
//
// No reference counterpart in /root/reference: the Groth16 wrap that answers GenFinalProof
// (proto/prover/v1/prover.proto:130-148, client src/prover/provider.rs:472-503) lives in the external
// prover.  Pippenger bucket method, window c bits:
//   1. digits     : counting sort of the point indices by window digit (histogram -> scan -> scatter)
//   2. bucket sums: one lane per (window, bucket) adds its points (Jacobian += affine, 7M+4S)
//   3. reduction  : running sums over segments of MSM_SEG buckets, segment weights by double-and-add,
//                   tree sum per window in LDS
//   4. the <= 32 window results are combined on the host (254 doublings).
// Field: F_q in Montgomery form, 9 x 29-bit limbs, product scanning with v_mad_u64_u32 (see below).  VALU only;
// the MFMA limb-product formulation north_star mentions is not built.
#include <hip/hip_runtime.h>

#include <type_traits>

#include <cstring>
#include <vector>

#include <thread>

#include "ctx.hpp"
#include "fq254.hpp"

namespace {

// ---- 1. sort of the point indices by window digit, two levels so that every global write lands next to its
// neighbours.  (The first version was one atomic counting sort: 4-byte writes to random addresses, 16x write
// amplification and a returning global atomic per (point, window) -- as slow as the bucket sums themselves.)
//   coarse digit = LOW `hi` bits of the window digit, fine digit = the `lo` bits above them (lo <= 10): skewed scalars
//   (many equal or tiny values, the short top window) then land in coarse bins that hold a single digit each, which
//   the fine stage handles with one LDS atomic per wave instead of 64 colliding ones
//   1a. msm_coarse_hist : LDS histogram per 4096-point tile -> counts[window][coarse]
//   1b. msm_scan        : exclusive scan per window -> coarse starts
//   1c. msm_coarse_part : per tile, LDS ranks + one global reservation per (window, coarse bin) -> (index, fine
//                         digit) pairs grouped by coarse bin (order inside a bin is arbitrary)
//   1d. msm_fine_sort   : one workgroup per (window, coarse bin): counting sort by fine digit with LDS counters,
//                         inside that bin's contiguous (L2-sized) region; also emits starts/counts per bucket
#define MSM_TILE 4096
#define MSM_LO_MAX 10
struct SortGeo {
    int c, hi, lo, nwin, wgroup;   // c = hi + lo: bucket-index bits of a window; wgroup: windows per pass of the tile kernels (LDS budget)
    int cd;                        // digit width = c + 1 (signed digits)
    u32 K[9];                      // the recoding bias  sum_w 2^(cd w + cd - 1)
};
__global__ void __launch_bounds__(256) msm_coarse_hist_kernel(const u32 *scalars, u64 n, SortGeo g, int w0, u32 *ccounts) {
    extern __shared__ u32 lh[];   // [wgroup][2^hi]
    const int nbin = 1 << g.hi, nw = min(g.wgroup, g.nwin - w0);
    for (int i = threadIdx.x; i < nw * nbin; i += 256) lh[i] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * MSM_TILE;
    for (int k = 0; k < MSM_TILE / 256; k++) {
        const u64 i = base + (u64)k * 256 + threadIdx.x;
        if (i < n) {
            u32 sc[8];
#pragma unroll
            for (int j = 0; j < 8; j++) sc[j] = scalars[i * 8 + j];
            u32 s9[9], neg;
            add_bias9(sc, g.K, s9);
            for (int w = 0; w < nw; w++) {
                const u32 d = digit_key(s9, w0 + w, g.cd, neg);
                if (d) atomicAdd(&lh[w * nbin + ((d - 1) & (nbin - 1))], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nw * nbin; i += 256)
        if (lh[i]) atomicAdd(&ccounts[(u64)(w0 + i / nbin) * nbin + (i % nbin)], lh[i]);
}
// exclusive scan of the 2^bits counters of one window (one block per window)
__global__ void __launch_bounds__(1024) msm_scan_kernel(const u32 *counts, u32 *starts, u32 *cursor, int bits) {
    __shared__ u32 part[1024];
    const u64 base = (u64)blockIdx.x << bits;
    const u32 nb = 1u << bits;
    const u32 per = (nb + 1023) / 1024;
    const u32 lo = min(threadIdx.x * per, nb), hi = min(lo + per, nb);
    u32 s = 0;
    for (u32 b = lo; b < hi; b++) s += counts[base + b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int t = 0; t < 1024; t++) {
            u32 v = part[t];
            part[t] = run;
            run += v;
        }
    }
    __syncthreads();
    u32 run = part[threadIdx.x];
    for (u32 b = lo; b < hi; b++) {
        starts[base + b] = run;
        cursor[base + b] = run;
        run += counts[base + b];
    }
}
__global__ void __launch_bounds__(256) msm_coarse_part_kernel(const u32 *scalars, u64 n, SortGeo g, int w0, u32 *ccursor,
                                                             u32 *pidx, u32 *pfine) {
    extern __shared__ u32 lh[];   // [wgroup][2^hi] counters, then [wgroup][2^hi] global bases
    const int nbin = 1 << g.hi, nw = min(g.wgroup, g.nwin - w0);
    u32 *lbase = lh + g.wgroup * nbin;
    for (int i = threadIdx.x; i < nw * nbin; i += 256) lh[i] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * MSM_TILE;
    for (int k = 0; k < MSM_TILE / 256; k++) {   // phase A: how many of this tile go to each (window, coarse bin)
        const u64 i = base + (u64)k * 256 + threadIdx.x;
        if (i < n) {
            u32 sc[8];
#pragma unroll
            for (int j = 0; j < 8; j++) sc[j] = scalars[i * 8 + j];
            u32 s9[9], neg;
            add_bias9(sc, g.K, s9);
            for (int w = 0; w < nw; w++) {
                const u32 d = digit_key(s9, w0 + w, g.cd, neg);
                if (d) atomicAdd(&lh[w * nbin + ((d - 1) & (nbin - 1))], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nw * nbin; i += 256) {   // one global reservation per (window, coarse bin) of the tile
        const u32 cnt = lh[i];
        lbase[i] = cnt ? atomicAdd(&ccursor[(u64)(w0 + i / nbin) * nbin + (i % nbin)], cnt) : 0u;
        lh[i] = 0;
    }
    __syncthreads();
    for (int k = 0; k < MSM_TILE / 256; k++) {   // phase B: rank inside the tile's share of the bin, write the pair
        const u64 i = base + (u64)k * 256 + threadIdx.x;
        if (i < n) {
            u32 sc[8];
#pragma unroll
            for (int j = 0; j < 8; j++) sc[j] = scalars[i * 8 + j];
            u32 s9[9], neg;
            add_bias9(sc, g.K, s9);
            for (int w = 0; w < nw; w++) {
                const u32 d = digit_key(s9, w0 + w, g.cd, neg);
                if (d) {
                    const int b = w * nbin + ((d - 1) & (nbin - 1));
                    const u32 pos = lbase[b] + atomicAdd(&lh[b], 1u);
                    pidx[(u64)(w0 + w) * n + pos] = (u32)i | (neg << 31);   // the sign of the digit travels with the index
                    pfine[(u64)(w0 + w) * n + pos] = (d - 1) >> g.hi;
                }
            }
        }
    }
}
// ---- 1d. fine stage, slice-parallel: a coarse bin is cut into slices of MSM_FSLICE elements, one workgroup each, so
// that a bin holding millions of elements (skewed scalars) is sorted by many workgroups.
//   msm_slices      : slice list (coarse bin, slice number) per (window, coarse bin)
//   msm_fine_hist   : LDS histogram of a slice by fine digit -> counts[bucket] (global atomics, one per digit present)
//   msm_fine_scan   : per coarse bin: exclusive scan of its <= 1024 bucket counts -> starts[bucket], cursor[bucket]
//   msm_fine_scatter: per slice: reserve cursor[bucket] once per digit present, rank in LDS, write the indices
// A wave whose 64 elements carry one and the same digit (the skewed case) issues one LDS atomic, not 64 colliding ones.
#define MSM_FSLICE 8192
__global__ void __launch_bounds__(256) msm_slices_kernel(const u32 *ccounts, u32 ncoarse, u32 *slice_count, uint2 *slices) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncoarse) return;
    const u32 cc = ccounts[i];
    const u32 nsl = (cc + MSM_FSLICE - 1) / MSM_FSLICE;
    if (!nsl) return;
    const u32 base = atomicAdd(slice_count, nsl);
    for (u32 s = 0; s < nsl; s++) slices[base + s] = make_uint2(i, s);
}
// LDS histogram of one slice by fine digit (cnt must be zero on entry, nf entries)
__device__ __forceinline__ void slice_hist(const u32 *pf, u32 lo, u32 hi, u32 *cnt) {
    const int lane = threadIdx.x & 63;
    for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
        const u32 f = pf[i];
        const u64 act = __ballot(1);
        if (__ballot(f == (u32)__builtin_amdgcn_readfirstlane((int)f)) == act) {   // one digit in the whole wave
            if (lane == __ffsll((long long)act) - 1) atomicAdd(&cnt[f], (u32)__popcll(act));
        } else {
            atomicAdd(&cnt[f], 1u);
        }
    }
}
__global__ void __launch_bounds__(256) msm_fine_hist_kernel(const u32 *pfine, u64 n, SortGeo g, const uint2 *slices,
                                                           const u32 *cstarts, const u32 *ccounts, u32 *counts) {
    __shared__ u32 cnt[1 << MSM_LO_MAX];
    const int nbin = 1 << g.hi, nf = 1 << g.lo;
    const uint2 sl = slices[blockIdx.x];
    const u64 w = sl.x / nbin, bin = sl.x % nbin;
    const u32 cs = cstarts[sl.x], cc = ccounts[sl.x];
    const u32 lo = sl.y * MSM_FSLICE, hi = min(lo + (u32)MSM_FSLICE, cc);
    for (int i = threadIdx.x; i < nf; i += 256) cnt[i] = 0;
    __syncthreads();
    slice_hist(pfine + w * n + cs, lo, hi, cnt);
    __syncthreads();
    for (int f = threadIdx.x; f < nf; f += 256)
        if (cnt[f]) atomicAdd(&counts[(w << g.c) + ((u64)f << g.hi) + bin], cnt[f]);
}
__global__ void __launch_bounds__(1024) msm_fine_scan_kernel(SortGeo g, const u32 *cstarts, const u32 *counts, u32 *starts,
                                                            u32 *cursor) {
    __shared__ u32 part[1024];
    const int nbin = 1 << g.hi, nf = 1 << g.lo;
    const u64 w = blockIdx.x / nbin, bin = blockIdx.x % nbin;
    const u32 cs = cstarts[blockIdx.x];
    const u64 bucket = (w << g.c) + ((u64)threadIdx.x << g.hi) + bin;
    const u32 mine = (int)threadIdx.x < nf ? counts[bucket] : 0u;
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const u32 v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    if ((int)threadIdx.x < nf) {
        const u32 at = cs + part[threadIdx.x] - mine;
        starts[bucket] = at;
        cursor[bucket] = at;
    }
}
__global__ void __launch_bounds__(256) msm_fine_scatter_kernel(const u32 *pidx, const u32 *pfine, u64 n, SortGeo g,
                                                              const uint2 *slices, const u32 *cstarts, const u32 *ccounts,
                                                              u32 *cursor, u32 *sorted) {
    __shared__ u32 cnt[1 << MSM_LO_MAX], lbase[1 << MSM_LO_MAX];
    const int nbin = 1 << g.hi, nf = 1 << g.lo;
    const uint2 sl = slices[blockIdx.x];
    const u64 w = sl.x / nbin, bin = sl.x % nbin;
    const u32 cs = cstarts[sl.x], cc = ccounts[sl.x];
    const u32 lo = sl.y * MSM_FSLICE, hi = min(lo + (u32)MSM_FSLICE, cc);
    const u32 *pi = pidx + w * n + cs, *pf = pfine + w * n + cs;
    for (int i = threadIdx.x; i < nf; i += 256) cnt[i] = 0;
    __syncthreads();
    slice_hist(pf, lo, hi, cnt);
    __syncthreads();
    for (int f = threadIdx.x; f < nf; f += 256) {   // one global reservation per digit present in the slice
        const u32 k = cnt[f];
        lbase[f] = k ? atomicAdd(&cursor[(w << g.c) + ((u64)f << g.hi) + bin], k) : 0u;
        cnt[f] = 0;
    }
    __syncthreads();
    u32 *out = sorted + w * n;
    const int lane = threadIdx.x & 63;
    for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
        const u32 f = pf[i];
        const u64 act = __ballot(1);
        u32 rank;
        if (__ballot(f == (u32)__builtin_amdgcn_readfirstlane((int)f)) == act) {
            u32 base = 0;
            if (lane == __ffsll((long long)act) - 1) base = atomicAdd(&cnt[f], (u32)__popcll(act));
            base = (u32)__builtin_amdgcn_readfirstlane((int)base);
            rank = base + (u32)__popcll(act & ((1ULL << lane) - 1));
        } else {
            rank = atomicAdd(&cnt[f], 1u);
        }
        out[lbase[f] + rank] = pi[i];
    }
}

// a packed affine point = 2 * FT<F>::WORDS words = NV uint4 (G1: 4, G2: 8); (0, 0) encodes the point at infinity
template <class F>
__device__ __forceinline__ void unpack_point(const uint4 *q, F &x, F &y) {
    constexpr int NV = FT<F>::WORDS / 2;
    u32 w[FT<F>::WORDS * 2];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        w[4 * k] = q[k].x;
        w[4 * k + 1] = q[k].y;
        w[4 * k + 2] = q[k].z;
        w[4 * k + 3] = q[k].w;
    }
    x = FT<F>::from_words(w);
    y = FT<F>::from_words(w + FT<F>::WORDS);
}
// ---- 2a. one-time conversion of the affine inputs to Montgomery form (16-byte vector accesses); stored packed
template <class F>
__global__ void __launch_bounds__(256) msm_to_mont_kernel(const uint4 *points, u64 n, uint4 *mont) {
    constexpr int NV = FT<F>::WORDS / 2;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint4 q[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) q[k] = points[i * NV + k];
    F x, y;
    unpack_point<F>(q, x, y);
    u32 w[FT<F>::WORDS * 2];
    FT<F>::to_words(f_to_mont(x), w);   // (0,0) stays (0,0): still the infinity marker
    FT<F>::to_words(f_to_mont(y), w + FT<F>::WORDS);
#pragma unroll
    for (int k = 0; k < NV; k++) mont[i * NV + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// ---- 2b. bucket sums: lane = (window, bucket).  Software pipeline, two points per trip: while point k is added,
// point k+1 and the index of point k+2 are in flight.  All loads are unconditional (indices clamped to the bucket's
// last point) so that no loop-carried register needs a copy under an exec mask -- with a conditional prefetch the
// compiler parked a v_mov (and therefore an s_waitcnt) right behind every load and nothing was overlapped.
template <class F>
__device__ __forceinline__ jacT<F> madd_packed(const jacT<F> &acc, const uint4 *q, u32 neg) {
    F x, y;
    unpack_point<F>(q, x, y);
    if (f_is_zero(x) && f_is_zero(y)) return acc;
    // negative digit: add -P = (x, -y)
    if constexpr (std::is_same<F, fq>::value) {
        if (neg) y = lz_sub<1>(fq_zero(), y);  // q - y in (0, q]: one carry pass
        return jac_madd_lazy(acc, x, y);       // unreduced between the products; canonical at the store
    } else {
        if (neg) y = f_sub(FT<F>::zero(), y);
        return jac_madd(acc, x, y);
    }
}
// Buckets with more than MSM_HEAVY points are not summed by one lane: real scalars are not uniform (the top window of
// a 254-bit scalar has 2-12 significant bits, witnesses are full of small values), and one lane walking a million points
// would take seconds.  Such a bucket is cut into chunks of MSM_HCHUNK points, each summed by a whole workgroup
// (msm_heavy_kernel), and the chunk sums are added per bucket (msm_heavy_combine_kernel).
#define MSM_HEAVY 256
#define MSM_HCHUNK 16384
struct HeavyLists {
    u32 *counters;   // [0] = chunks appended, [1] = heavy buckets appended
    uint2 *chunks;   // (bucket id, chunk number)
    uint4 *heavy;    // (bucket id, first chunk slot, number of chunks, 0)
};
// Lanes of a wave sum buckets of EQUAL size: a wave runs as long as its largest bucket, and with ~4-64 points per bucket (Poisson) the largest
// of 64 is 1.3-1.6 times the mean -- that much of the bucket kernel was lanes waiting.  The (window, bucket) ids are therefore counting-sorted by
// their point count, largest first (bin MSM_HEAVY + 1: the heavy buckets, which only append to the heavy lists), and lane i takes order[i].
//   msm_order_hist : histogram of min(count, MSM_HEAVY + 1) over all buckets (LDS, then one global atomic per bin and block)
//   msm_order_scan : exclusive scan from the largest bin down (one block)
//   msm_order_fill : rank inside the block (LDS), one reservation per bin and block, order[pos] = id
#define MSM_OBINS (MSM_HEAVY + 2)
__global__ void __launch_bounds__(256) msm_order_hist_kernel(const u32 *counts, u64 nb, u32 *hist) {
    __shared__ u32 h[MSM_OBINS];
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256) h[i] = 0;
    __syncthreads();
    for (u64 id = (u64)blockIdx.x * 256 + threadIdx.x; id < nb; id += (u64)gridDim.x * 256) {
        const u32 cnt = counts[id];
        atomicAdd(&h[cnt > MSM_HEAVY ? MSM_HEAVY + 1 : cnt], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
__global__ void __launch_bounds__(64) msm_order_scan_kernel(const u32 *hist, u32 *cursor) {
    if (threadIdx.x) return;
    u32 run = 0;
    for (int b = MSM_OBINS - 1; b >= 0; b--) { cursor[b] = run; run += hist[b]; }
}
__global__ void __launch_bounds__(256) msm_order_fill_kernel(const u32 *counts, u64 nb, u32 *cursor, u32 *order) {
    __shared__ u32 h[MSM_OBINS], base[MSM_OBINS];
    const u64 id = (u64)blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256) h[i] = 0;
    __syncthreads();
    u32 bin = 0, rank = 0;
    if (id < nb) {
        const u32 cnt = counts[id];
        bin = cnt > MSM_HEAVY ? MSM_HEAVY + 1 : cnt;
        rank = atomicAdd(&h[bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256)
        if (h[i]) base[i] = atomicAdd(&cursor[i], h[i]);
    __syncthreads();
    if (id < nb) order[base[bin] + rank] = (u32)id;
}
template <class F>
__global__ void __launch_bounds__(256) msm_bucket_kernel(const uint4 *mont, u64 n, int c, int nwin, const u32 *starts,
                                                        const u32 *counts, const u32 *sorted, const u32 *order, jacT<F> *buckets, HeavyLists hl) {
    constexpr int NV = FT<F>::WORDS / 2;
    const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x;
    if (gid >= ((u64)nwin << c)) return;
    const u64 id = order[gid];
    const u64 w = id >> c;
    const u32 st = starts[id], cnt = counts[id];
    if (cnt > MSM_HEAVY) {
        const u32 nch = (cnt + MSM_HCHUNK - 1) / MSM_HCHUNK;
        const u32 slot = atomicAdd(&hl.counters[0], nch);
        for (u32 k = 0; k < nch; k++) hl.chunks[slot + k] = make_uint2((u32)id, k);
        hl.heavy[atomicAdd(&hl.counters[1], 1u)] = make_uint4((u32)id, slot, nch, 0u);
        return;
    }
    const u32 *idx = sorted + w * n + st;
    jacT<F> acc = jac_inf<F>();
    if (cnt) {
        const u32 last = cnt - 1;
        uint4 A[NV], B[NV];
        u32 va = idx[0];                     // bit 31: sign of the digit, bits 0..30: point index
        u64 pa = va & 0x7FFFFFFFu;
#pragma unroll
        for (int j = 0; j < NV; j++) A[j] = mont[pa * NV + j];
        u32 ia = idx[last < 1 ? last : 1];
        for (u32 k = 0; k < cnt; k += 2) {
            const u32 vb = ia;
            const u64 pb = vb & 0x7FFFFFFFu;
#pragma unroll
            for (int j = 0; j < NV; j++) B[j] = mont[pb * NV + j];
            const u32 ib = idx[k + 2 < last ? k + 2 : last];
            acc = madd_packed<F>(acc, A, va >> 31);
            va = ib;
            pa = va & 0x7FFFFFFFu;
#pragma unroll
            for (int j = 0; j < NV; j++) A[j] = mont[pa * NV + j];
            ia = idx[k + 3 < last ? k + 3 : last];
            if (k + 1 < cnt) acc = madd_packed<F>(acc, B, vb >> 31);
        }
    }
    buckets[id] = jac_canon(acc);
}
// one workgroup per chunk of a heavy bucket: lane t sums points t, t+256, ... of the chunk, LDS tree over the lanes
template <class F>
__global__ void __launch_bounds__(256) msm_heavy_kernel(const uint4 *mont, u64 n, int c, const u32 *starts, const u32 *counts,
                                                       const u32 *sorted, HeavyLists hl, jacT<F> *partial) {
    constexpr int NV = FT<F>::WORDS / 2;
    __shared__ jacT<F> sh[256];
    const uint2 ch = hl.chunks[blockIdx.x];
    const u64 id = ch.x, w = id >> c;
    const u32 cnt = counts[id];
    const u32 lo = ch.y * MSM_HCHUNK, hi = min(lo + (u32)MSM_HCHUNK, cnt);
    const u32 *idx = sorted + w * n + starts[id];
    jacT<F> acc = jac_inf<F>();
    for (u32 k = lo + threadIdx.x; k < hi; k += 256) {
        const u32 vi = idx[k];
        const u64 pi = vi & 0x7FFFFFFFu;
        uint4 q[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) q[j] = mont[pi * NV + j];
        acc = madd_packed<F>(acc, q, vi >> 31);
    }
    sh[threadIdx.x] = jac_canon(acc);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = jac_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
// one wave per heavy bucket: lane t adds chunk sums t, t+64, ..., LDS tree over the lanes
template <class F>
__global__ void __launch_bounds__(64) msm_heavy_combine_kernel(HeavyLists hl, u32 nheavy, const jacT<F> *partial, jacT<F> *buckets) {
    __shared__ jacT<F> sh[64];
    const uint4 h = hl.heavy[blockIdx.x];
    jacT<F> acc = jac_inf<F>();
    for (u32 k = threadIdx.x; k < h.z; k += 64) acc = jac_add(acc, partial[h.y + k]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = jac_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) buckets[h.x] = sh[0];
}
// ---- 3a. per segment of SEG buckets: sum_{b in seg} (b + 1) * B_b   (bucket index b holds the points of digit magnitude b + 1)
// (round 6: 16 instead of 64 -- the kernel is one dependent chain of additions per lane with fewer lanes than the chip has SIMD slots:
// four times the lanes at a third of the chain, 2.2 -> 0.6 ms per 2^24-point run)
#define MSM_SEG 16
template <class F>
__global__ void __launch_bounds__(64) msm_segment_kernel(const jacT<F> *buckets, int c, int nwin, jacT<F> *segs) {
    const u64 id = (u64)blockIdx.x * 64 + threadIdx.x;
    const u64 segs_per_win = (1ULL << c) / MSM_SEG;
    if (id >= (u64)nwin * segs_per_win) return;
    const u64 w = id / segs_per_win, sidx = id % segs_per_win;
    const u64 s = sidx * MSM_SEG;
    const jacT<F> *B = buckets + (w << c) + s;
    jacT<F> run = jac_inf<F>(), acc = jac_inf<F>();
    for (int k = MSM_SEG - 1; k >= 1; k--) {
        run = jac_add(run, B[k]);
        acc = jac_add(acc, run);
    }
    run = jac_add(run, B[0]);                       // total of the segment
    acc = jac_add(acc, jac_mul_small(run, (u32)s + 1));     // + (s + 1) * total
    segs[id] = acc;
}
// ---- 3b. tree sum of the segment results of one window (one block per window)
template <class F>
__global__ void __launch_bounds__(256) msm_window_kernel(const jacT<F> *segs, int nseg, jacT<F> *wins) {
    __shared__ jacT<F> sh[256];
    const jacT<F> *S = segs + (u64)blockIdx.x * nseg;
    jacT<F> acc = jac_inf<F>();
    for (int k = threadIdx.x; k < nseg; k += 256) acc = jac_add(acc, S[k]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = jac_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) wins[blockIdx.x] = sh[0];
}

// All scratch of a run comes from ONE ctx-owned arena that only grows: hipMalloc/hipFree of gigabytes per call cost
// up to 45 ms (more than the 2^22-point run itself) once the process holds other large allocations.
static int32_t msm_arena(zp_ctx *ctx, size_t bytes, char **out) {
    if (ctx->msm_arena_bytes < bytes) {
        if (ctx->msm_arena) {
            ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            ZP_HIP(ctx, hipFree(ctx->msm_arena));
            ctx->msm_arena = nullptr;
            ctx->msm_arena_bytes = 0;
        }
        ZP_HIP(ctx, hipMalloc(&ctx->msm_arena, bytes));
        ctx->msm_arena_bytes = bytes;
    }
    *out = (char *)ctx->msm_arena;
    return ZP_OK;
}

// one Pippenger run over n points (n <= 2^24 from the entry points): result as a Jacobian point in *out
template <class F>
int32_t msm_chunk(zp_ctx *ctx, const uint32_t *d_points, const uint32_t *d_scalars, size_t n, jacT<F> *out) {
    constexpr int NV = FT<F>::WORDS / 2;
    using J = jacT<F>;
    int c = 4;
    while (c < 16 && (1ULL << (c + 2)) <= n) c++;   // ~4 points per bucket up to c = 16
    while (c < 20 && (1ULL << (c + 8)) <= n) c++;   // wider windows only while buckets keep >= 128 points (signed digits: profiles/r2_msm_c_sweep.txt)
    if (ctx->tune_msm_c > 0) c = ctx->tune_msm_c;    // experiment knob
    if (c < 6) c = 6;                                // segments of MSM_SEG buckets (and the sort geometry) need c >= 6
    if (c > 22) c = 22;
    // c = bucket-index bits of a window; digits are signed and one bit wider (cd = c + 1).  s + K must stay below 2^(cd nwin)
    // for any 256-bit scalar (the BN254 group order has 254 bits): cd * nwin >= 258
    const int cd = c + 1;
    const int nwin = (258 + cd - 1) / cd;
    const u64 nb = (u64)nwin << c;
    u32 *d_counts = nullptr, *d_starts = nullptr, *d_sorted = nullptr;
    J *d_buckets = nullptr, *d_segs = nullptr, *d_wins = nullptr;
    uint4 *d_mont = nullptr;
    const u64 nseg = (1ULL << c) / MSM_SEG;
    SortGeo g;
    g.c = c;
    g.lo = c < MSM_LO_MAX ? c : MSM_LO_MAX;
    g.hi = c - g.lo;
    g.nwin = nwin;
    g.cd = cd;
    for (int j = 0; j < 9; j++) g.K[j] = 0;
    for (int w = 0; w < nwin; w++) {
        const int bit = cd * w + cd - 1;            // < 288
        g.K[bit >> 5] |= 1u << (bit & 31);
    }
    g.wgroup = nwin;
    while ((size_t)g.wgroup * ((size_t)2 << g.hi) * sizeof(u32) > 48 * 1024 && g.wgroup > 1) g.wgroup = (g.wgroup + 1) / 2;
    const u64 ncoarse = (u64)nwin << g.hi;
    ZP_HIP(ctx, hipSetDevice(ctx->device));
    // arena layout (256-byte aligned pieces): per-bucket counts/starts/cursor | coarse counts/starts/cursor | slice list |
    // sorted indices + coarse-partitioned (index, fine) pairs | Montgomery points | buckets/segments/windows | heavy lists | chunk sums
    const u64 max_slices = (u64)nwin * n / MSM_FSLICE + ncoarse + 1;
    const u64 max_heavy = (u64)nwin * n / MSM_HEAVY + 1, max_chunks = (u64)nwin * n / MSM_HCHUNK + max_heavy + 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t sz_counts = al((nb * 4 + 2 * MSM_OBINS + ncoarse * 3 + 8 + max_slices * 2) * 4), sz_sorted = al((u64)nwin * n * 4 * 3),
                 sz_mont = al((u64)n * NV * 16), sz_buckets = al((nb + nwin * nseg + nwin) * sizeof(J)),
                 sz_hl = al(16 + max_chunks * sizeof(uint2) + max_heavy * sizeof(uint4)), sz_partial = al(max_chunks * sizeof(J));
    char *arena = nullptr;
    ZP_TRY(msm_arena(ctx, sz_counts + sz_sorted + sz_mont + sz_buckets + sz_hl + sz_partial, &arena));
    d_counts = (u32 *)arena;
    d_sorted = (u32 *)(arena + sz_counts);
    d_mont = (uint4 *)(arena + sz_counts + sz_sorted);
    d_buckets = (J *)(arena + sz_counts + sz_sorted + sz_mont);
    u32 *d_hl = (u32 *)(arena + sz_counts + sz_sorted + sz_mont + sz_buckets);
    J *d_partial = (J *)(arena + sz_counts + sz_sorted + sz_mont + sz_buckets + sz_hl);
    d_starts = d_counts + nb;
    u32 *d_fcursor = d_starts + nb;
    u32 *d_order = d_fcursor + nb, *d_ohist = d_order + nb;     // bucket ids sorted by size | MSM_OBINS histogram bins, then as many cursors
    u32 *d_ccounts = d_ohist + 2 * MSM_OBINS, *d_cstarts = d_ccounts + ncoarse, *d_ccursor = d_cstarts + ncoarse;
    u32 *d_slice_count = d_ccursor + ncoarse;
    uint2 *d_slices = (uint2 *)(((uintptr_t)(d_slice_count + 4) + 7) & ~(uintptr_t)7);
    u32 *d_pidx = d_sorted + (u64)nwin * n, *d_pfine = d_pidx + (u64)nwin * n;
    d_segs = d_buckets + nb;
    d_wins = d_segs + nwin * nseg;
    ZP_HIP(ctx, hipMemsetAsync(d_ccounts, 0, (ncoarse * 3 + 4) * 4, ctx->stream));   // coarse counters + slice count
    const unsigned gb = (unsigned)((n + 255) / 256), gt = (unsigned)((n + MSM_TILE - 1) / MSM_TILE);
    hipLaunchKernelGGL(msm_to_mont_kernel<F>, dim3(gb), dim3(256), 0, ctx->stream, (const uint4 *)d_points, (u64)n, d_mont);
    const size_t lds1 = (size_t)g.wgroup * ((size_t)1 << g.hi) * sizeof(u32);
    for (int w0 = 0; w0 < nwin; w0 += g.wgroup)
        hipLaunchKernelGGL(msm_coarse_hist_kernel, dim3(gt), dim3(256), lds1, ctx->stream, (const u32 *)d_scalars, (u64)n, g, w0, d_ccounts);
    hipLaunchKernelGGL(msm_scan_kernel, dim3(nwin), dim3(1024), 0, ctx->stream, d_ccounts, d_cstarts, d_ccursor, g.hi);
    for (int w0 = 0; w0 < nwin; w0 += g.wgroup)
        hipLaunchKernelGGL(msm_coarse_part_kernel, dim3(gt), dim3(256), 2 * lds1, ctx->stream, (const u32 *)d_scalars, (u64)n, g, w0,
                           d_ccursor, d_pidx, d_pfine);
    // fine stage: slice list on the device, its length read back (one of the two host round trips of a run)
    hipLaunchKernelGGL(msm_slices_kernel, dim3((unsigned)((ncoarse + 255) / 256)), dim3(256), 0, ctx->stream, d_ccounts, (u32)ncoarse,
                       d_slice_count, d_slices);
    u32 nslices = 0;
    hipError_t he = hipMemcpyAsync(&nslices, d_slice_count, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    if (he == hipSuccess) he = hipMemsetAsync(d_counts, 0, nb * 4, ctx->stream);
    if (he == hipSuccess && nslices)
        hipLaunchKernelGGL(msm_fine_hist_kernel, dim3(nslices), dim3(256), 0, ctx->stream, d_pfine, (u64)n, g, d_slices, d_cstarts,
                           d_ccounts, d_counts);
    if (he == hipSuccess)
        hipLaunchKernelGGL(msm_fine_scan_kernel, dim3((unsigned)ncoarse), dim3(1024), 0, ctx->stream, g, d_cstarts, d_counts, d_starts,
                           d_fcursor);
    if (he == hipSuccess && nslices)
        hipLaunchKernelGGL(msm_fine_scatter_kernel, dim3(nslices), dim3(256), 0, ctx->stream, d_pidx, d_pfine, (u64)n, g, d_slices,
                           d_cstarts, d_ccounts, d_fcursor, d_sorted);
    if (he == hipSuccess) he = hipMemsetAsync(d_ohist, 0, 2 * MSM_OBINS * 4, ctx->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(msm_order_hist_kernel, dim3(256), dim3(256), 0, ctx->stream, (const u32 *)d_counts, nb, d_ohist);
        hipLaunchKernelGGL(msm_order_scan_kernel, dim3(1), dim3(64), 0, ctx->stream, (const u32 *)d_ohist, d_ohist + MSM_OBINS);
        hipLaunchKernelGGL(msm_order_fill_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)d_counts, nb, d_ohist + MSM_OBINS, d_order);
    }
    HeavyLists hl;
    hl.counters = d_hl;
    hl.heavy = (uint4 *)(d_hl + 4);
    hl.chunks = (uint2 *)(hl.heavy + max_heavy);
    ZP_HIP(ctx, hipMemsetAsync(d_hl, 0, 16, ctx->stream));
    hipLaunchKernelGGL(msm_bucket_kernel<F>, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint4 *)d_mont, (u64)n, c, nwin, d_starts, d_counts, d_sorted, (const u32 *)d_order, d_buckets, hl);
    u32 hcnt[2] = {0, 0};
    if (he == hipSuccess) he = hipMemcpyAsync(hcnt, d_hl, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
    if (he == hipSuccess && hcnt[0]) {
        {
            hipLaunchKernelGGL(msm_heavy_kernel<F>, dim3(hcnt[0]), dim3(256), 0, ctx->stream, (const uint4 *)d_mont, (u64)n, c, d_starts,
                               d_counts, d_sorted, hl, d_partial);
            hipLaunchKernelGGL(msm_heavy_combine_kernel<F>, dim3(hcnt[1]), dim3(64), 0, ctx->stream, hl, hcnt[1], d_partial,
                               d_buckets);
        }
    }
    hipLaunchKernelGGL(msm_segment_kernel<F>, dim3((unsigned)((nwin * nseg + 63) / 64)), dim3(64), 0, ctx->stream, d_buckets, c, nwin, d_segs);
    hipLaunchKernelGGL(msm_window_kernel<F>, dim3(nwin), dim3(256), 0, ctx->stream, d_segs, (int)nseg, d_wins);
    hipError_t le = hipGetLastError();
    std::vector<J> wins(nwin);
    hipError_t ce = hipMemcpyAsync(wins.data(), d_wins, nwin * sizeof(J), hipMemcpyDeviceToHost, ctx->stream);
    hipError_t se = hipStreamSynchronize(ctx->stream);
    ZP_HIP(ctx, he);
    ZP_HIP(ctx, le);
    ZP_HIP(ctx, ce);
    ZP_HIP(ctx, se);
    // host: sum_w 2^(cd*w) * W_w  (Horner from the top window)
    J acc = jac_inf<F>();
    for (int w = nwin - 1; w >= 0; w--) {
        for (int k = 0; k < cd; k++) acc = jac_dbl(acc);
        acc = jac_add(acc, wins[w]);
    }
    *out = acc;
    return ZP_OK;
}

// Points are processed in runs of 2^24 (G1: 1 GiB of points): the bucket kernel reads points at random, and beyond
// that footprint its rate halves (2^26 in one run: 3.7 G additions/s against 8.1 G/s at 2^24); the partial sums are
// added on the host.
#define MSM_CHUNK_LOG 24
// a Jacobian sum as affine words in the layout of the entry points (standard form; infinity leaves h_out as it is: the callers zero it)
template <class F>
void jac_to_words(const jacT<F> &acc, uint32_t *h_out) {
    if (f_is_zero(acc.Z)) return;  // infinity: all-zero output
    F zi = f_inv_host(acc.Z);
    F zi2 = f_sqr(zi);
    F x = f_from_mont(f_mul(acc.X, zi2));
    F y = f_from_mont(f_mul(acc.Y, f_mul(zi2, zi)));
    FT<F>::to_words(x, h_out);
    FT<F>::to_words(y, h_out + FT<F>::WORDS);
}

template <class F>
int32_t msm_run(zp_ctx *ctx, const uint32_t *d_points, const uint32_t *d_scalars, size_t n, uint32_t *h_out) {
    constexpr int PW = FT<F>::WORDS * 2;   // words per affine point
    ZP_ARG(ctx, h_out != nullptr, "null output");
    ZP_ARG(ctx, n < (1ULL << 31), "too many points");
    memset(h_out, 0, PW * sizeof(uint32_t));
    if (n == 0) return ZP_OK;
    ZP_ARG(ctx, d_points && d_scalars, "null device pointer");
    jacT<F> acc = jac_inf<F>();
    const size_t chunk = (size_t)1 << (ctx->tune_msm_chunk_log > 0 ? ctx->tune_msm_chunk_log : MSM_CHUNK_LOG);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t len = n - off < chunk ? n - off : chunk;
        jacT<F> part;
        ZP_TRY(msm_chunk<F>(ctx, d_points + off * PW, d_scalars + off * 8, len, &part));
        acc = jac_add(acc, part);
    }
    jac_to_words(acc, h_out);
    return ZP_OK;
}

// ---- sharded MSM: rank r sums its slice of the points (the rule of zpi_shard_range) with msm_run, the world partial sums travel as affine words in
// ONE all-gather, and every rank adds them in rank order on the host.  The affine sum is unique: every rank returns what zp_msm_bn254 / _g2 returns
// for the whole input on one ctx, word for word.
template <class F>
int32_t msm_sharded(zp_comm *comm, const uint32_t *d_points, const uint32_t *d_scalars, size_t n_total, uint32_t *h_out) {
    constexpr int PW = FT<F>::WORDS * 2;   // u32 per affine point: PW / 2 u64 words per rank in the exchange
    zp_ctx *ctx = zpi_comm_ctx(comm);
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, PW == 16 ? "msm_bn254_sharded" : "msm_bn254_g2_sharded");
    const int world = zp_comm_world(comm), rank = zp_comm_rank(comm);
    size_t first = 0, count = 0;
    zpi_shard_range(n_total, world, rank, &first, &count);
    const size_t xbytes = (size_t)(world + 1) * PW * 4;
    void *d_x = nullptr;
    int32_t rc = ZP_OK;
    try {
        std::vector<uint32_t> parts((size_t)world * PW, 0);
        if (!h_out || n_total >= (1ULL << 31) || (count && !(d_points && d_scalars))) {
            ctx->err = "bad argument: null output or slice, or too many points";
            rc = ZP_ERR_ARG;
        }
        if (rc == ZP_OK) rc = msm_run<F>(ctx, d_points, d_scalars, count, parts.data());       // an empty slice: infinity
        if (rc == ZP_OK) rc = zpi_pool_alloc(ctx, xbytes, &d_x);
        if (rc == ZP_OK) rc = zpi_h2d_small(ctx, d_x, parts.data(), PW * 4);
        if (rc == ZP_OK) rc = zp_comm_all_gather(comm, (const uint64_t *)d_x, (uint64_t *)d_x + PW / 2, PW / 2);
        if (rc == ZP_OK) rc = zpi_d2h_small(ctx, parts.data(), (const uint64_t *)d_x + PW / 2, (size_t)world * PW * 4);
        if (d_x) zpi_pool_release(ctx, d_x, xbytes);
        if (rc != ZP_OK) return zpi_comm_fail(comm, rc);
        zpi_bn254_affine_sum(PW == 32, parts.data(), world, h_out);
        return ZP_OK;
    } catch (...) {
        if (d_x) zpi_pool_release(ctx, d_x, xbytes);
        ctx->err = "out of host memory in a sharded MSM";
        return zpi_comm_fail(comm, ZP_ERR_NOMEM);
    }
}

template <class F>
void affine_sum(const uint32_t *pts, int count, uint32_t *out) {
    constexpr int W = FT<F>::WORDS;
    jacT<F> acc = jac_inf<F>();
    for (int i = 0; i < count; i++) {
        const uint32_t *p = pts + (size_t)i * 2 * W;
        bool inf = true;
        for (int k = 0; k < 2 * W; k++) inf = inf && p[k] == 0;
        if (inf) continue;
        jacT<F> q;
        q.X = f_to_mont(FT<F>::from_words(p));
        q.Y = f_to_mont(FT<F>::from_words(p + W));
        q.Z = FT<F>::one();
        acc = jac_add(acc, q);
    }
    memset(out, 0, 2 * W * sizeof(uint32_t));
    jac_to_words(acc, out);
}

}  // namespace

void zpi_bn254_affine_sum(int g2, const uint32_t *pts, int count, uint32_t *out) {
    if (g2) affine_sum<fq2>(pts, count, out);
    else affine_sum<fq>(pts, count, out);
}

extern "C" int32_t zp_msm_bn254(zp_ctx *ctx, const uint32_t *d_points, const uint32_t *d_scalars, size_t n,
                                uint32_t *h_out) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "msm_bn254");
    return msm_run<fq>(ctx, d_points, d_scalars, n, h_out);
}

extern "C" int32_t zp_msm_bn254_g2(zp_ctx *ctx, const uint32_t *d_points, const uint32_t *d_scalars, size_t n,
                                   uint32_t *h_out) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "msm_bn254_g2");
    return msm_run<fq2>(ctx, d_points, d_scalars, n, h_out);
}

extern "C" int32_t zp_msm_bn254_sharded(zp_comm *comm, const uint32_t *d_points_local, const uint32_t *d_scalars_local, size_t n_total, uint32_t *h_out) {
    return msm_sharded<fq>(comm, d_points_local, d_scalars_local, n_total, h_out);
}

extern "C" int32_t zp_msm_bn254_g2_sharded(zp_comm *comm, const uint32_t *d_points_local, const uint32_t *d_scalars_local, size_t n_total, uint32_t *h_out) {
    return msm_sharded<fq2>(comm, d_points_local, d_scalars_local, n_total, h_out);
}

// ---- fixed-base multiplication: out_i = s_i * B for ONE base B -- the group elements of a Groth16 key ([u_j(tau)]_1, [v_j(tau)]_2, ...: millions of
// scalars times the generator; zp_r1cs_key_scalars makes the scalars).  An MSM sums; this does not.  Table T[w][d] = d 2^(8w) B (32 windows of
// 8 bits, 255 entries each, affine, Montgomery form, built on the host with one batched inversion), lane = scalar: 32 table additions
// (Jacobian += affine), result stored in Jacobian form; the host turns the results affine with batched inversions on threads (one field
// inversion per 1 024 points) and writes them in the layout zp_msm_bn254 / _g2 read.  Setup work: run once per key, not per proof.
namespace {

template <class F>
__global__ void __launch_bounds__(256) fixed_base_kernel(const uint4 *__restrict__ table, const u32 *__restrict__ scalars, u64 n, jacT<F> *__restrict__ out) {
    constexpr int NV = FT<F>::WORDS / 2;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 sc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) sc[k] = scalars[i * 8 + k];
    jacT<F> acc = jac_inf<F>();
    for (int w = 0; w < 32; w++) {
        const u32 d = (sc[w >> 2] >> (8 * (w & 3))) & 255u;
        if (d == 0) continue;
        uint4 q[NV];
        const uint4 *src = table + ((size_t)w * 256 + d) * NV;
#pragma unroll
        for (int k = 0; k < NV; k++) q[k] = src[k];
        F x, y;
        unpack_point<F>(q, x, y);
        acc = jac_madd(acc, x, y);
    }
    out[i] = acc;
}

// Jacobian -> affine, standard form, packed words ((0, 0) for the point at infinity): Montgomery's trick over runs of `run` points
template <class F>
void batch_to_affine_host(const jacT<F> *pts, size_t n, u32 *out_words, int threads) {
    constexpr int W2 = 2 * FT<F>::WORDS;
    const size_t run = 1024, nrun = (n + run - 1) / run;
    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    if (T < 1) T = 1;
    if (T > 32) T = 32;
    if ((size_t)T > nrun) T = (int)(nrun ? nrun : 1);
    auto work = [&](size_t r0, size_t r1) {
        std::vector<F> pre(run);
        for (size_t r = r0; r < r1; r++) {
            const size_t a = r * run, b = a + run < n ? a + run : n;
            F acc = FT<F>::one();
            for (size_t i = a; i < b; i++) {
                pre[i - a] = acc;
                if (!f_is_zero(pts[i].Z)) acc = f_mul(acc, pts[i].Z);
            }
            F inv = f_inv_host(acc);
            for (size_t i = b; i-- > a;) {
                u32 *o = out_words + i * W2;
                if (f_is_zero(pts[i].Z)) { memset(o, 0, W2 * 4); continue; }
                const F zi = f_mul(inv, pre[i - a]);          // 1 / Z_i
                inv = f_mul(inv, pts[i].Z);
                const F zi2 = f_sqr(zi);
                FT<F>::to_words(f_from_mont(f_mul(pts[i].X, zi2)), o);
                FT<F>::to_words(f_from_mont(f_mul(pts[i].Y, f_mul(zi2, zi))), o + FT<F>::WORDS);
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++) {
        const size_t r0 = nrun * t / T, r1 = nrun * (t + 1) / T;
        if (r0 < r1) pool.emplace_back(work, r0, r1);
    }
    for (auto &th : pool) th.join();
}

template <class F>
int32_t fixed_base_run(zp_ctx *ctx, const uint32_t *h_base, const uint32_t *h_scalars, size_t n, uint32_t *h_points, int32_t threads) {
    constexpr int NV = FT<F>::WORDS / 2, W2 = 2 * FT<F>::WORDS;
    ZP_ARG(ctx, h_base && (n == 0 || (h_scalars && h_points)), "null pointer");
    if (n == 0) return ZP_OK;
    F bx = f_to_mont(FT<F>::from_words(h_base)), by = f_to_mont(FT<F>::from_words(h_base + FT<F>::WORDS));
    ZP_ARG(ctx, !(f_is_zero(bx) && f_is_zero(by)), "the base is the point at infinity");
    // the table in Jacobian form on the host: T[w][d] = T[w][d - 1] + B_w, B_(w+1) = 256 B_w
    std::vector<jacT<F>> tab((size_t)32 * 256);
    jacT<F> bw;
    bw.X = bx; bw.Y = by; bw.Z = FT<F>::one();
    for (int w = 0; w < 32; w++) {
        tab[(size_t)w * 256] = jac_inf<F>();
        for (int d = 1; d < 256; d++) tab[(size_t)w * 256 + d] = jac_add(tab[(size_t)w * 256 + d - 1], bw);
        bw = jac_add(tab[(size_t)w * 256 + 255], bw);
    }
    std::vector<u32> tw(tab.size() * W2), tm(tab.size() * W2);
    batch_to_affine_host<F>(tab.data(), tab.size(), tw.data(), threads);
    for (size_t e = 0; e < tab.size(); e++) {       // back to Montgomery form, the kernel's input (infinity stays (0, 0))
        FT<F>::to_words(f_to_mont(FT<F>::from_words(&tw[e * W2])), &tm[e * W2]);
        FT<F>::to_words(f_to_mont(FT<F>::from_words(&tw[e * W2 + FT<F>::WORDS])), &tm[e * W2 + FT<F>::WORDS]);
    }
    void *d_tab = nullptr, *d_sc = nullptr, *d_out = nullptr;
    int32_t rc = zp_dev_alloc(ctx, tm.size() * 4, &d_tab);
    if (rc == ZP_OK) rc = zp_dev_alloc(ctx, n * 32, &d_sc);
    if (rc == ZP_OK) rc = zp_dev_alloc(ctx, n * sizeof(jacT<F>), &d_out);
    if (rc == ZP_OK) rc = zp_h2d(ctx, d_tab, tm.data(), tm.size() * 4);
    if (rc == ZP_OK) rc = zp_h2d(ctx, d_sc, h_scalars, n * 32);
    std::vector<jacT<F>> res;
    if (rc == ZP_OK) {
        hipLaunchKernelGGL(fixed_base_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4 *)d_tab, (const u32 *)d_sc, (u64)n,
                           (jacT<F> *)d_out);
        if (hipGetLastError() != hipSuccess) { ctx->err = "fixed_base_kernel launch failed"; rc = ZP_ERR_HIP; }
        (void)NV;
    }
    if (rc == ZP_OK) {
        res.resize(n);
        rc = zp_d2h(ctx, res.data(), d_out, n * sizeof(jacT<F>));
    }
    if (d_tab) (void)zp_dev_free(ctx, d_tab);
    if (d_sc) (void)zp_dev_free(ctx, d_sc);
    if (d_out) (void)zp_dev_free(ctx, d_out);
    if (rc != ZP_OK) return rc;
    batch_to_affine_host<F>(res.data(), n, h_points, threads);
    return ZP_OK;
}

}  // namespace

extern "C" int32_t zp_fixed_base_mul_bn254(zp_ctx *ctx, const uint32_t *h_base, const uint32_t *h_scalars, size_t n, uint32_t *h_points, int32_t threads) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "fixed_base_mul_bn254");
    try {
        return fixed_base_run<fq>(ctx, h_base, h_scalars, n, h_points, threads);
    } catch (...) {
        ctx->err = "out of host memory";
        return ZP_ERR_NOMEM;
    }
}

extern "C" int32_t zp_fixed_base_mul_bn254_g2(zp_ctx *ctx, const uint32_t *h_base, const uint32_t *h_scalars, size_t n, uint32_t *h_points, int32_t threads) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "fixed_base_mul_bn254_g2");
    try {
        return fixed_base_run<fq2>(ctx, h_base, h_scalars, n, h_points, threads);
    } catch (...) {
        ctx->err = "out of host memory";
        return ZP_ERR_NOMEM;
    }
}

// ---- synthetic MSM inputs: n DISTINCT points P_i = (start + i) * G of BN254 G1 (host code, this file's own field
// arithmetic).  Like zp_synth_trace it stands in for data the offline build cannot obtain (a real proving key); distinct
// points make an MSM benchmark read 64 B per point from HBM instead of hitting a small table in cache, and the known
// discrete logs give a checkable answer: sum_i s_i P_i = (sum_i s_i (start + i) mod r) * G.
// Affine chord additions P_base + j*G against a table of 1024 multiples, one batched inversion per block.
namespace {
struct affp { fq x, y; };
affp aff_add_host(const affp &p, const affp &q) {   // p != -q
    fq num, den;
    if (fq_eq(p.x, q.x)) {
        const fq t = fq_sqr(p.x);
        num = fq_add(fq_add(t, t), t);
        den = fq_add(p.y, p.y);
    } else {
        num = fq_sub(q.y, p.y);
        den = fq_sub(q.x, p.x);
    }
    const fq lam = fq_mul(num, fq_inv_host(den));
    affp r;
    r.x = fq_sub(fq_sub(fq_sqr(lam), p.x), q.x);
    r.y = fq_sub(fq_mul(lam, fq_sub(p.x, r.x)), p.y);
    return r;
}
affp aff_mul_g_host(const affp &g, u64 k) {   // k >= 1
    affp acc = g, base = g;
    bool started = false;
    for (int i = 0; i < 64 && (k >> i); i++) {
        if ((k >> i) & 1) {
            acc = started ? aff_add_host(acc, base) : base;
            started = true;
        }
        base = aff_add_host(base, base);
    }
    return acc;
}
void aff_store(uint32_t *out, const affp &p) {
    fq_to_words(fq_from_mont(p.x), out);
    fq_to_words(fq_from_mont(p.y), out + 8);
}
}  // namespace

#include <thread>
extern "C" int32_t zp_synth_g1_points(uint64_t start, size_t n, uint32_t *h_points, int32_t threads) {
    constexpr int BLK = 1024;
    if (!h_points || start <= (uint64_t)BLK || start + n < start) return ZP_ERR_ARG;
    if (n == 0) return ZP_OK;
    affp g;
    {
        fq one = fq_zero(), two = fq_zero();
        one.l[0] = 1;
        two.l[0] = 2;
        g.x = fq_to_mont(one);
        g.y = fq_to_mont(two);
    }
    std::vector<affp> tab(BLK + 1);   // tab[j] = j*G
    tab[1] = g;
    for (int j = 2; j <= BLK; j++) tab[j] = aff_add_host(tab[j - 1], g);
    const size_t nblk = (n + BLK - 1) / BLK;
    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    if (T < 1) T = 1;
    if ((size_t)T > nblk) T = (int)nblk;
    auto work = [&](size_t b0, size_t b1) {
        std::vector<fq> den(BLK), pre(BLK);
        affp base = aff_mul_g_host(g, start + b0 * BLK);
        for (size_t b = b0; b < b1; b++) {
            const size_t cnt = (b + 1) * BLK <= n ? BLK : n - b * BLK;
            uint32_t *o = h_points + b * BLK * 16;
            aff_store(o, base);
            fq acc = fq_one();
            for (int j = 1; j <= BLK; j++) {
                den[j - 1] = fq_sub(tab[j].x, base.x);
                pre[j - 1] = acc;
                acc = fq_mul(acc, den[j - 1]);
            }
            fq inv = fq_inv_host(acc);
            affp next = base;
            for (int j = BLK; j >= 1; j--) {
                const fq dinv = fq_mul(inv, pre[j - 1]);
                inv = fq_mul(inv, den[j - 1]);
                if ((size_t)j >= cnt && j != BLK) continue;
                const fq lam = fq_mul(fq_sub(tab[j].y, base.y), dinv);
                affp r;
                r.x = fq_sub(fq_sub(fq_sqr(lam), base.x), tab[j].x);
                r.y = fq_sub(fq_mul(lam, fq_sub(base.x, r.x)), base.y);
                if (j == BLK) next = r;
                if ((size_t)j < cnt) aff_store(o + (size_t)j * 16, r);
            }
            base = next;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++) {
        const size_t b0 = nblk * t / T, b1 = nblk * (t + 1) / T;
        if (b0 < b1) pool.emplace_back(work, b0, b1);
    }
    for (auto &th : pool) th.join();
    return ZP_OK;
}
