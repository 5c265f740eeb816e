// BN254 (alt_bn128) multi-scalar multiplication over G1 and G2: sum_i s_i * P_i   (SURVEY.md 8a N6).  This file holds the MSM and nothing else:
// the fixed-base multiplication of the key setup is csrc/fixed_base.hip, the synthetic input points are csrc/synth.hip.
//
// No reference counterpart in /root/reference: the Groth16 wrap that answers GenFinalProof
// (proto/prover/v1/prover.proto:130-148, client src/prover/provider.rs:472-503) lives in the external
// prover.  Pippenger bucket method, window c bits:
//   1. digits     : counting sort of the point indices by window digit (histogram -> scan -> scatter)
//   2. bucket sums: one lane per (window, bucket) adds its points (Jacobian += affine, 7M+4S)
//   3. reduction  : running sums over segments of MSM_SEG buckets, segment weights by double-and-add,
//                   tree sum per window in LDS
//   4. the <= 32 window results are combined on the host (254 doublings).
// Field and curve code: csrc/fq254.hpp (F_q in Montgomery form, 9 x 29-bit limbs).  VALU only; the MFMA limb-product formulation north_star
// mentions is not built.
// Written once, used by every kernel that needs it: tile_digits (the walk over a tile's window digits), wave_count (LDS counter, one atomic per
// wave of equal keys), reserve_bins (one global reservation per bin and block), block_exclusive_scan, block_jac_sum, entry_* (the sorted entry).
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>
#include <vector>

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
//   1c. msm_coarse_part : per tile, LDS ranks + one global reservation per (window, coarse bin) -> (entry, fine
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
// a digit of magnitude d >= 1 belongs to bucket d - 1 of its window: coarse bin = its low hi bits, fine digit = the lo bits above
__device__ __forceinline__ u32 coarse_bin(const SortGeo &g, u32 d) { return (d - 1) & ((1u << g.hi) - 1); }
__device__ __forceinline__ u32 fine_digit(const SortGeo &g, u32 d) { return (d - 1) >> g.hi; }
__device__ __forceinline__ u64 bucket_of(const SortGeo &g, u64 w, u64 bin, u64 fine) { return (w << g.c) + (fine << g.hi) + bin; }
// a sorted entry: the point index with the sign of its digit in bit 31 (n < 2^31)
__device__ __forceinline__ u32 entry_make(u32 index, u32 neg) { return index | (neg << 31); }
__device__ __forceinline__ u32 entry_index(u32 e) { return e & 0x7FFFFFFFu; }
__device__ __forceinline__ u32 entry_neg(u32 e) { return e >> 31; }

// the digit walk of one tile (block) in one pass over windows w0 .. w0 + nw - 1: fn(i, w, d, neg) for every non-zero digit -- point i, window
// w0 + w, magnitude d, sign neg
template <class Fn>
__device__ __forceinline__ void tile_digits(const u32 *scalars, u64 n, const SortGeo &g, int w0, int nw, Fn fn) {
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
                if (d) fn(i, w, d, neg);
            }
        }
    }
}
// cnt[key] += 1 from every active lane, returning the lane's rank among the block's elements of that key so far.  A wave whose active lanes
// all carry ONE key (skewed scalars) issues one LDS atomic, not 64 colliding ones.  A caller that only counts ignores the rank, and the compiler drops its computation.
__device__ __forceinline__ u32 wave_count(u32 *cnt, u32 key) {
    const int lane = threadIdx.x & 63;
    const u64 act = __ballot(1);
    if (__ballot(key == (u32)__builtin_amdgcn_readfirstlane((int)key)) == act) {
        u32 base = 0;
        if (lane == __ffsll((long long)act) - 1) base = atomicAdd(&cnt[key], (u32)__popcll(act));
        base = (u32)__builtin_amdgcn_readfirstlane((int)base);
        return base + (u32)__popcll(act & ((1ULL << lane) - 1));
    }
    return atomicAdd(&cnt[key], 1u);
}
// the reservation step of a counting sort whose blocks counted into LDS: one global atomic per bin that holds something,
// base[b] = where this block's share of bin b starts; the counters go back to zero for the ranking pass.  256 threads.
template <class Cursor>
__device__ __forceinline__ void reserve_bins(u32 *cnt, u32 *base, int nbins, Cursor cursor_of) {
    for (int b = threadIdx.x; b < nbins; b += 256) {
        const u32 k = cnt[b];
        base[b] = k ? atomicAdd(cursor_of(b), k) : 0u;
        cnt[b] = 0;
    }
}
// exclusive scan of count(0) .. count(n - 1) by one block of NT threads: a thread owns a run of ceil(n / NT) consecutive items, the runs'
// totals are scanned in LDS (Hillis-Steele) and put(j, sum of the counts before j) is called for every item
template <int NT, class Count, class Put>
__device__ __forceinline__ void block_exclusive_scan(u32 n, Count count, Put put) {
    __shared__ u32 part[NT];
    const u32 t = threadIdx.x, per = (n + NT - 1) / NT;
    const u32 lo = min(t * per, n), hi = min(lo + per, n);
    u32 s = 0;
    for (u32 j = lo; j < hi; j++) s += count(j);
    part[t] = s;
    __syncthreads();
    for (u32 d = 1; d < NT; d <<= 1) {
        const u32 v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u32 run = part[t] - s;
    for (u32 j = lo; j < hi; j++) {
        put(j, run);
        run += count(j);
    }
}
// LDS tree sum of one Jacobian point per lane over the N lanes of the block; lane 0 stores the total to *out
template <class F, int N>
__device__ __forceinline__ void block_jac_sum(const jacT<F> &mine, jacT<F> *out) {
    __shared__ jacT<F> sh[N];
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = jac_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

__global__ void __launch_bounds__(256) msm_coarse_hist_kernel(const u32 *scalars, u64 n, SortGeo g, int w0, u32 *ccounts) {
    extern __shared__ u32 lh[];   // [wgroup][2^hi]
    const int nbin = 1 << g.hi, nw = min(g.wgroup, g.nwin - w0);
    for (int i = threadIdx.x; i < nw * nbin; i += 256) lh[i] = 0;
    __syncthreads();
    tile_digits(scalars, n, g, w0, nw, [&](u64, int w, u32 d, u32) { atomicAdd(&lh[w * nbin + coarse_bin(g, d)], 1u); });
    __syncthreads();
    for (int i = threadIdx.x; i < nw * nbin; i += 256)
        if (lh[i]) atomicAdd(&ccounts[(u64)w0 * nbin + i], lh[i]);
}
// exclusive scan of the 2^bits counters of one window (one block per window)
__global__ void __launch_bounds__(1024) msm_scan_kernel(const u32 *counts, u32 *starts, u32 *cursor, int bits) {
    const u64 base = (u64)blockIdx.x << bits;
    block_exclusive_scan<1024>(1u << bits, [&](u32 b) { return counts[base + b]; }, [&](u32 b, u32 at) {
        starts[base + b] = at;
        cursor[base + b] = at;
    });
}
__global__ void __launch_bounds__(256) msm_coarse_part_kernel(const u32 *scalars, u64 n, SortGeo g, int w0, u32 *ccursor,
                                                             u32 *pidx, u32 *pfine) {
    extern __shared__ u32 lh[];   // [wgroup][2^hi] counters, then [wgroup][2^hi] global bases
    const int nbin = 1 << g.hi, nw = min(g.wgroup, g.nwin - w0);
    u32 *lbase = lh + g.wgroup * nbin;
    for (int i = threadIdx.x; i < nw * nbin; i += 256) lh[i] = 0;
    __syncthreads();
    // phase A: how many of this tile go to each (window, coarse bin)
    tile_digits(scalars, n, g, w0, nw, [&](u64, int w, u32 d, u32) { atomicAdd(&lh[w * nbin + coarse_bin(g, d)], 1u); });
    __syncthreads();
    reserve_bins(lh, lbase, nw * nbin, [&](int b) { return &ccursor[(u64)w0 * nbin + b]; });
    __syncthreads();
    // phase B: rank inside the tile's share of the bin, write the pair
    tile_digits(scalars, n, g, w0, nw, [&](u64 i, int w, u32 d, u32 neg) {
        const int b = w * nbin + coarse_bin(g, d);
        const u32 pos = lbase[b] + atomicAdd(&lh[b], 1u);
        pidx[(u64)(w0 + w) * n + pos] = entry_make((u32)i, neg);
        pfine[(u64)(w0 + w) * n + pos] = fine_digit(g, d);
    });
}
// ---- 1d. fine stage, slice-parallel: a coarse bin is cut into slices of MSM_FSLICE elements, one workgroup each, so
// that a bin holding millions of elements (skewed scalars) is sorted by many workgroups.
//   msm_slices      : slice list (coarse bin, slice number) per (window, coarse bin)
//   msm_fine_hist   : LDS histogram of a slice by fine digit -> counts[bucket] (global atomics, one per digit present)
//   msm_fine_scan   : per coarse bin: exclusive scan of its <= 1024 bucket counts -> starts[bucket], cursor[bucket]
//   msm_fine_scatter: per slice: reserve cursor[bucket] once per digit present, rank in LDS, write the entries
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
// what a block of the fine stage works on: elements lo .. hi - 1 of coarse bin `bin` of window w, whose region starts at element cs of the window
struct FineSlice {
    u64 w, bin;
    u32 cs, lo, hi;
};
__device__ __forceinline__ FineSlice fine_slice(const SortGeo &g, const uint2 *slices, const u32 *cstarts, const u32 *ccounts) {
    const uint2 sl = slices[blockIdx.x];   // (window * 2^hi + coarse bin, slice number)
    const u32 lo = sl.y * MSM_FSLICE;
    return FineSlice{sl.x >> g.hi, sl.x & ((1u << g.hi) - 1), cstarts[sl.x], lo, min(lo + (u32)MSM_FSLICE, ccounts[sl.x])};
}
// LDS histogram of the block's slice by fine digit (cnt: 2^lo entries, zeroed here)
__device__ __forceinline__ void slice_hist(const SortGeo &g, const u32 *pf, const FineSlice &s, u32 *cnt) {
    for (int i = threadIdx.x; i < (1 << g.lo); i += 256) cnt[i] = 0;
    __syncthreads();
    for (u32 i = s.lo + threadIdx.x; i < s.hi; i += 256) (void)wave_count(cnt, pf[i]);
    __syncthreads();
}
__global__ void __launch_bounds__(256) msm_fine_hist_kernel(const u32 *pfine, u64 n, SortGeo g, const uint2 *slices,
                                                           const u32 *cstarts, const u32 *ccounts, u32 *counts) {
    __shared__ u32 cnt[1 << MSM_LO_MAX];
    const FineSlice s = fine_slice(g, slices, cstarts, ccounts);
    slice_hist(g, pfine + s.w * n + s.cs, s, cnt);
    for (int f = threadIdx.x; f < (1 << g.lo); f += 256)
        if (cnt[f]) atomicAdd(&counts[bucket_of(g, s.w, s.bin, f)], cnt[f]);
}
__global__ void __launch_bounds__(1024) msm_fine_scan_kernel(SortGeo g, const u32 *cstarts, const u32 *counts, u32 *starts,
                                                            u32 *cursor) {
    const u64 w = blockIdx.x >> g.hi, bin = blockIdx.x & ((1u << g.hi) - 1);
    const u32 cs = cstarts[blockIdx.x];
    block_exclusive_scan<1024>(1u << g.lo, [&](u32 f) { return counts[bucket_of(g, w, bin, f)]; }, [&](u32 f, u32 at) {
        starts[bucket_of(g, w, bin, f)] = cs + at;
        cursor[bucket_of(g, w, bin, f)] = cs + at;
    });
}
__global__ void __launch_bounds__(256) msm_fine_scatter_kernel(const u32 *pidx, const u32 *pfine, u64 n, SortGeo g,
                                                              const uint2 *slices, const u32 *cstarts, const u32 *ccounts,
                                                              u32 *cursor, u32 *sorted) {
    __shared__ u32 cnt[1 << MSM_LO_MAX], lbase[1 << MSM_LO_MAX];
    const FineSlice s = fine_slice(g, slices, cstarts, ccounts);
    const u32 *pi = pidx + s.w * n + s.cs, *pf = pfine + s.w * n + s.cs;
    slice_hist(g, pf, s, cnt);
    reserve_bins(cnt, lbase, 1 << g.lo, [&](int f) { return &cursor[bucket_of(g, s.w, s.bin, f)]; });
    __syncthreads();
    u32 *out = sorted + s.w * n;
    for (u32 i = s.lo + threadIdx.x; i < s.hi; i += 256) {
        const u32 f = pf[i];
        const u32 rank = wave_count(cnt, f);
        out[lbase[f] + rank] = pi[i];
    }
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
__device__ __forceinline__ u32 order_bin(u32 count) { return count > MSM_HEAVY ? MSM_HEAVY + 1 : count; }
__global__ void __launch_bounds__(256) msm_order_hist_kernel(const u32 *counts, u64 nb, u32 *hist) {
    __shared__ u32 h[MSM_OBINS];
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256) h[i] = 0;
    __syncthreads();
    for (u64 id = (u64)blockIdx.x * 256 + threadIdx.x; id < nb; id += (u64)gridDim.x * 256) atomicAdd(&h[order_bin(counts[id])], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
__global__ void __launch_bounds__(64) msm_order_scan_kernel(const u32 *hist, u32 *cursor) {   // item j of the scan is bin MSM_OBINS - 1 - j
    block_exclusive_scan<64>(MSM_OBINS, [&](u32 j) { return hist[MSM_OBINS - 1 - j]; }, [&](u32 j, u32 at) { cursor[MSM_OBINS - 1 - j] = at; });
}
__global__ void __launch_bounds__(256) msm_order_fill_kernel(const u32 *counts, u64 nb, u32 *cursor, u32 *order) {
    __shared__ u32 h[MSM_OBINS], base[MSM_OBINS];
    const u64 id = (u64)blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < MSM_OBINS; i += 256) h[i] = 0;
    __syncthreads();
    u32 bin = 0, rank = 0;
    if (id < nb) {
        bin = order_bin(counts[id]);
        rank = atomicAdd(&h[bin], 1u);
    }
    __syncthreads();
    reserve_bins(h, base, MSM_OBINS, [&](int b) { return &cursor[b]; });
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
        u32 va = idx[0];
        u64 pa = entry_index(va);
#pragma unroll
        for (int j = 0; j < NV; j++) A[j] = mont[pa * NV + j];
        u32 ia = idx[last < 1 ? last : 1];
        for (u32 k = 0; k < cnt; k += 2) {
            const u32 vb = ia;
            const u64 pb = entry_index(vb);
#pragma unroll
            for (int j = 0; j < NV; j++) B[j] = mont[pb * NV + j];
            const u32 ib = idx[k + 2 < last ? k + 2 : last];
            acc = madd_packed<F>(acc, A, entry_neg(va));
            va = ib;
            pa = entry_index(va);
#pragma unroll
            for (int j = 0; j < NV; j++) A[j] = mont[pa * NV + j];
            ia = idx[k + 3 < last ? k + 3 : last];
            if (k + 1 < cnt) acc = madd_packed<F>(acc, B, entry_neg(vb));
        }
    }
    buckets[id] = jac_canon(acc);
}
// one workgroup per chunk of a heavy bucket: lane t sums points t, t+256, ... of the chunk, LDS tree over the lanes
template <class F>
__global__ void __launch_bounds__(256) msm_heavy_kernel(const uint4 *mont, u64 n, int c, const u32 *starts, const u32 *counts,
                                                       const u32 *sorted, HeavyLists hl, jacT<F> *partial) {
    constexpr int NV = FT<F>::WORDS / 2;
    const uint2 ch = hl.chunks[blockIdx.x];
    const u64 id = ch.x, w = id >> c;
    const u32 cnt = counts[id];
    const u32 lo = ch.y * MSM_HCHUNK, hi = min(lo + (u32)MSM_HCHUNK, cnt);
    const u32 *idx = sorted + w * n + starts[id];
    jacT<F> acc = jac_inf<F>();
    for (u32 k = lo + threadIdx.x; k < hi; k += 256) {
        const u32 e = idx[k];
        const u64 pi = entry_index(e);
        uint4 q[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) q[j] = mont[pi * NV + j];
        acc = madd_packed<F>(acc, q, entry_neg(e));
    }
    block_jac_sum<F, 256>(jac_canon(acc), &partial[blockIdx.x]);
}
// one wave per heavy bucket: lane t adds chunk sums t, t+64, ..., LDS tree over the lanes
template <class F>
__global__ void __launch_bounds__(64) msm_heavy_combine_kernel(HeavyLists hl, const jacT<F> *partial, jacT<F> *buckets) {
    const uint4 h = hl.heavy[blockIdx.x];
    jacT<F> acc = jac_inf<F>();
    for (u32 k = threadIdx.x; k < h.z; k += 64) acc = jac_add(acc, partial[h.y + k]);
    block_jac_sum<F, 64>(acc, &buckets[h.x]);
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
    const jacT<F> *S = segs + (u64)blockIdx.x * nseg;
    jacT<F> acc = jac_inf<F>();
    for (int k = threadIdx.x; k < nseg; k += 256) acc = jac_add(acc, S[k]);
    block_jac_sum<F, 256>(acc, &wins[blockIdx.x]);
}

// ---- host side of one Pippenger run, top to bottom: window width -> sort geometry -> arena plan -> three enqueue stages -> Horner
// window width (bucket-index bits c) for a run of n points; `knob` > 0 dictates it (zp_set_tuning "msm_c")
int msm_window_bits(size_t n, int knob) {
    int c = 4;
    while (c < 16 && (1ULL << (c + 2)) <= n) c++;   // ~4 points per bucket up to c = 16
    while (c < 20 && (1ULL << (c + 8)) <= n) c++;   // wider windows only while buckets keep >= 128 points (signed digits: profiles/r2_msm_c_sweep.txt)
    if (knob > 0) c = knob;                          // experiment knob
    if (c < 6) c = 6;                                // segments of MSM_SEG buckets (and the sort geometry) need c >= 6
    if (c > 22) c = 22;
    return c;
}
// c = bucket-index bits of a window; digits are signed and one bit wider (cd = c + 1).  s + K must stay below 2^(cd nwin)
// for any 256-bit scalar (the BN254 group order has 254 bits): cd * nwin >= 258
SortGeo msm_sort_geo(int c) {
    SortGeo g;
    g.c = c;
    g.cd = c + 1;
    g.nwin = (258 + g.cd - 1) / g.cd;
    g.lo = c < MSM_LO_MAX ? c : MSM_LO_MAX;
    g.hi = c - g.lo;
    for (int j = 0; j < 9; j++) g.K[j] = 0;
    for (int w = 0; w < g.nwin; w++) {
        const int bit = g.cd * w + g.cd - 1;        // < 288
        g.K[bit >> 5] |= 1u << (bit & 31);
    }
    // windows per pass of the tile kernels: counters and bases of a pass, 2 * wgroup * 2^hi words, within 48 KiB of LDS
    g.wgroup = g.nwin;
    while ((size_t)g.wgroup * ((size_t)2 << g.hi) * sizeof(u32) > 48 * 1024 && g.wgroup > 1) g.wgroup = (g.wgroup + 1) / 2;
    return g;
}

// All scratch of a run comes from ONE ctx-owned arena that only grows: hipMalloc/hipFree of gigabytes per call cost
// up to 45 ms (more than the 2^22-point run itself) once the process holds other large allocations.
int32_t msm_arena(zp_ctx *ctx, size_t bytes, char **out) {
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
// carves pieces off one allocation, each at its type's alignment; over a null base it only measures (`at` ends as the size)
struct Bump {
    char *base;
    size_t at = 0;
    void align(size_t a) { at = (at + a - 1) & ~(a - 1); }
    template <class T>
    void take(T *&p, size_t count) {
        align(alignof(T));
        p = base ? (T *)(base + at) : nullptr;
        at += count * sizeof(T);
    }
};
// the arena of one run: ONE list of pieces gives the size (null base) and the pointers.  Six groups, each starting on a 256-byte boundary.
template <class F>
struct MsmPlan {
    size_t n, nb, ncoarse, nseg, max_slices, max_heavy, max_chunks;
    uint2 *slices;                                   // fine-stage slice list
    u32 *counts, *starts, *fcursor, *order;          // per bucket: point count, start in `sorted`, scatter cursor | bucket ids by size
    u32 *ohist;                                      // MSM_OBINS histogram bins of the size ordering, then as many cursors
    u32 *ccounts, *cstarts, *ccursor, *slice_count;  // per (window, coarse bin), then the length of the slice list: cleared by one memset
    u32 *sorted, *pidx, *pfine;                      // sorted entries | coarse-partitioned (entry, fine digit) pairs
    uint4 *mont;                                     // the points in Montgomery form
    jacT<F> *buckets, *segs, *wins;
    HeavyLists hl;
    jacT<F> *partial;                                // chunk sums of the heavy buckets
    size_t bytes;

    MsmPlan(size_t n_, const SortGeo &g, char *base) : n(n_) {
        constexpr int NV = FT<F>::WORDS / 2;
        nb = (size_t)g.nwin << g.c;
        ncoarse = (size_t)g.nwin << g.hi;
        nseg = ((size_t)1 << g.c) / MSM_SEG;
        max_slices = (size_t)g.nwin * n / MSM_FSLICE + ncoarse + 1;
        max_heavy = (size_t)g.nwin * n / MSM_HEAVY + 1;
        max_chunks = (size_t)g.nwin * n / MSM_HCHUNK + max_heavy + 1;
        Bump b{base};
        b.take(slices, max_slices);                  // the 8-byte piece first: the words behind it need no padding
        b.take(counts, nb);
        b.take(starts, nb);
        b.take(fcursor, nb);
        b.take(order, nb);
        b.take(ohist, 2 * MSM_OBINS);
        b.take(ccounts, ncoarse);
        b.take(cstarts, ncoarse);
        b.take(ccursor, ncoarse);
        b.take(slice_count, 8);                      // (one word used)
        b.align(256);
        b.take(sorted, (size_t)g.nwin * n);
        b.take(pidx, (size_t)g.nwin * n);
        b.take(pfine, (size_t)g.nwin * n);
        b.align(256);
        b.take(mont, n * NV);
        b.align(256);
        b.take(buckets, nb);
        b.take(segs, g.nwin * nseg);
        b.take(wins, g.nwin);
        b.align(256);
        b.take(hl.counters, 4);
        b.take(hl.heavy, max_heavy);
        b.take(hl.chunks, max_chunks);
        b.align(256);
        b.take(partial, max_chunks);
        b.align(256);
        bytes = b.at;
    }
};

// The enqueue stages return the first HIP error and launch nothing after it; msm_chunk drains the stream whatever they return.
#define MSM_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
#define MSM_LAUNCH(kernel, grid, block, lds, stream, ...) \
    do { hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, __VA_ARGS__); MSM_HIP(hipGetLastError()); } while (0)
inline unsigned blocks_of(size_t items, size_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// stage 1: points to Montgomery form; sorted entries, starts and counts per bucket; bucket ids ordered by size
template <class F>
hipError_t msm_enqueue_sort(hipStream_t st, const uint32_t *d_points, const u32 *d_scalars, const SortGeo &g, const MsmPlan<F> &p) {
    const u64 n = p.n;
    MSM_HIP(hipMemsetAsync(p.ccounts, 0, (size_t)((char *)(p.slice_count + 4) - (char *)p.ccounts), st));   // coarse counters + slice count
    MSM_LAUNCH(msm_to_mont_kernel<F>, blocks_of(n, 256), 256, 0, st, (const uint4 *)d_points, n, p.mont);
    const unsigned tiles = blocks_of(n, MSM_TILE);
    const size_t lds1 = (size_t)g.wgroup * ((size_t)1 << g.hi) * sizeof(u32);
    for (int w0 = 0; w0 < g.nwin; w0 += g.wgroup) MSM_LAUNCH(msm_coarse_hist_kernel, tiles, 256, lds1, st, d_scalars, n, g, w0, p.ccounts);
    MSM_LAUNCH(msm_scan_kernel, g.nwin, 1024, 0, st, p.ccounts, p.cstarts, p.ccursor, g.hi);
    for (int w0 = 0; w0 < g.nwin; w0 += g.wgroup)
        MSM_LAUNCH(msm_coarse_part_kernel, tiles, 256, 2 * lds1, st, d_scalars, n, g, w0, p.ccursor, p.pidx, p.pfine);
    // fine stage: slice list on the device, its length read back (one of the two host round trips of a run)
    MSM_LAUNCH(msm_slices_kernel, blocks_of(p.ncoarse, 256), 256, 0, st, p.ccounts, (u32)p.ncoarse, p.slice_count, p.slices);
    u32 nslices = 0;
    MSM_HIP(hipMemcpyAsync(&nslices, p.slice_count, 4, hipMemcpyDeviceToHost, st));
    MSM_HIP(hipStreamSynchronize(st));
    MSM_HIP(hipMemsetAsync(p.counts, 0, p.nb * 4, st));
    if (nslices) MSM_LAUNCH(msm_fine_hist_kernel, nslices, 256, 0, st, p.pfine, n, g, p.slices, p.cstarts, p.ccounts, p.counts);
    MSM_LAUNCH(msm_fine_scan_kernel, (unsigned)p.ncoarse, 1024, 0, st, g, p.cstarts, p.counts, p.starts, p.fcursor);
    if (nslices)
        MSM_LAUNCH(msm_fine_scatter_kernel, nslices, 256, 0, st, p.pidx, p.pfine, n, g, p.slices, p.cstarts, p.ccounts, p.fcursor, p.sorted);
    MSM_HIP(hipMemsetAsync(p.ohist, 0, 2 * MSM_OBINS * 4, st));
    MSM_LAUNCH(msm_order_hist_kernel, 256, 256, 0, st, p.counts, p.nb, p.ohist);
    MSM_LAUNCH(msm_order_scan_kernel, 1, 64, 0, st, p.ohist, p.ohist + MSM_OBINS);
    MSM_LAUNCH(msm_order_fill_kernel, blocks_of(p.nb, 256), 256, 0, st, p.counts, p.nb, p.ohist + MSM_OBINS, p.order);
    return hipSuccess;
}
// stage 2: bucket sums; the heavy buckets' lists are read back (the second host round trip) and summed by workgroups
template <class F>
hipError_t msm_enqueue_buckets(hipStream_t st, const SortGeo &g, const MsmPlan<F> &p) {
    const u64 n = p.n;
    MSM_HIP(hipMemsetAsync(p.hl.counters, 0, 16, st));
    MSM_LAUNCH(msm_bucket_kernel<F>, blocks_of(p.nb, 256), 256, 0, st, p.mont, n, g.c, g.nwin, p.starts, p.counts, p.sorted, p.order, p.buckets, p.hl);
    u32 hcnt[2] = {0, 0};   // chunks, heavy buckets
    MSM_HIP(hipMemcpyAsync(hcnt, p.hl.counters, 8, hipMemcpyDeviceToHost, st));
    MSM_HIP(hipStreamSynchronize(st));
    if (hcnt[0]) {
        MSM_LAUNCH(msm_heavy_kernel<F>, hcnt[0], 256, 0, st, p.mont, n, g.c, p.starts, p.counts, p.sorted, p.hl, p.partial);
        MSM_LAUNCH(msm_heavy_combine_kernel<F>, hcnt[1], 64, 0, st, p.hl, p.partial, p.buckets);
    }
    return hipSuccess;
}
// stage 3: segment sums, one tree sum per window, the window results to the host (read after the caller's synchronise)
template <class F>
hipError_t msm_enqueue_reduce(hipStream_t st, const SortGeo &g, const MsmPlan<F> &p, jacT<F> *h_wins) {
    MSM_LAUNCH(msm_segment_kernel<F>, blocks_of(g.nwin * p.nseg, 64), 64, 0, st, p.buckets, g.c, g.nwin, p.segs);
    MSM_LAUNCH(msm_window_kernel<F>, g.nwin, 256, 0, st, p.segs, (int)p.nseg, p.wins);
    MSM_HIP(hipMemcpyAsync(h_wins, p.wins, g.nwin * sizeof(jacT<F>), hipMemcpyDeviceToHost, st));
    return hipSuccess;
}
// host: sum_w 2^(cd w) * W_w  (Horner from the top window)
template <class F>
jacT<F> msm_horner(const std::vector<jacT<F>> &wins, int cd) {
    jacT<F> acc = jac_inf<F>();
    for (size_t w = wins.size(); w-- > 0;) {
        for (int k = 0; k < cd; k++) acc = jac_dbl(acc);
        acc = jac_add(acc, wins[w]);
    }
    return acc;
}

// one Pippenger run over n points (n <= 2^24 from the entry points): result as a Jacobian point in *out
template <class F>
int32_t msm_chunk(zp_ctx *ctx, const uint32_t *d_points, const uint32_t *d_scalars, size_t n, jacT<F> *out) {
    const SortGeo g = msm_sort_geo(msm_window_bits(n, ctx->tune_msm_c));
    ZP_HIP(ctx, hipSetDevice(ctx->device));
    char *arena = nullptr;
    ZP_TRY(msm_arena(ctx, MsmPlan<F>(n, g, nullptr).bytes, &arena));
    const MsmPlan<F> plan(n, g, arena);
    std::vector<jacT<F>> wins(g.nwin);
    hipError_t enqueue = msm_enqueue_sort<F>(ctx->stream, d_points, d_scalars, g, plan);
    if (enqueue == hipSuccess) enqueue = msm_enqueue_buckets<F>(ctx->stream, g, plan);
    if (enqueue == hipSuccess) enqueue = msm_enqueue_reduce<F>(ctx->stream, g, plan, wins.data());
    const hipError_t drain = hipStreamSynchronize(ctx->stream);   // also after a failure: the next call reuses the arena
    ZP_HIP(ctx, enqueue);
    ZP_HIP(ctx, drain);
    *out = msm_horner<F>(wins, g.cd);
    return ZP_OK;
}

// Points are processed in runs of 2^24 (G1: 1 GiB of points): the bucket kernel reads points at random, and beyond
// that footprint its rate halves (2^26 in one run: 3.7 G additions/s against 8.1 G/s at 2^24); the partial sums are
// added on the host.
#define MSM_CHUNK_LOG 24
// a Jacobian sum as affine words in the layout of the entry points (standard form; infinity leaves h_out as it is: the callers zero it)
template <class F>
void jac_to_words(const jacT<F> &acc, uint32_t *h_out) {
    if (!f_is_zero(acc.Z)) jac_affine_words(acc, f_inv_host(acc.Z), h_out);
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
