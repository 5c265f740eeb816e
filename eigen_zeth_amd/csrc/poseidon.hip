// Poseidon-12 over Goldilocks, linear-hash leaves and binary Merkle trees.
//
// No reference counterpart in /root/reference (hashing happens inside the external prover service
// that src/prover/provider.rs:358-377 calls).  Schedule ARK -> S-box(x^7) -> MDS, 4 full + 22 partial + 4 full
// rounds, tables injected through zp_set_constants.  The field values are the textbook's; on the default matrix the
// throughput kernels walk the partial rounds three at a time (partial3_default: three S-boxes + ONE matrix product,
// round 6) and compute only the digest rows of the last product where only a digest is read.
//
// Two mappings, each written once:
//   * throughput -- poseidon_perm<DEFMDS, OUT4>: one lane = one permutation, the 12-element state lives in 24 VGPRs; round constants and the MDS
//     matrix are wave-uniform and are fetched with scalar loads.  Kernels: poseidon_perm_kernel, merkle_leaves_kernel (one kernel for leaves given
//     as columns or as rows: the layout is a template argument), merkle_level_kernel, openings_lane_kernel, pow_grind_kernel.  Each exists for
//     the default matrix (literals) and for an injected one (LDS); launch_mds is the one place that picks between them.
//   * latency -- spread_perm: one lane = one state WORD, 12 lanes exchange a state through a 12-word LDS row.  Kernels: poseidon_perm_small_kernel,
//     the single-wave kernels through wave12_perm (poseidon_sponge_kernel, sponge_chains_kernel, openings_walk_kernel), merkle_leaves_coop_kernel
//     and merkle_subtree_kernel.  Any matrix, read as data.
// rowsum_reduce is the end of every row sum over a matrix that is data (mds_ark's general branch, spread_perm, poseidon_trace_kernel).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <type_traits>

#include "ctx.hpp"
// the Poseidon kernels fit 64 VGPRs (8 waves per SIMD) with the literal-table MDS: low scratch window
#define GL_ASM_SCRATCH_BASE 52
#include "gl_asm.hpp"

namespace {

// x^7 (any u64 in, weak out): the hand-scheduled 15-instruction weak products of gl_asm.hpp -- hipcc's gl_mul_weak is ~28 instructions,
// a third of them moves that build zero-extended 64-bit addends
__device__ __forceinline__ u64 sbox7(u64 x) {
    const u64 x2 = gl_mul1w(x, x);
    u64 x4 = x2, x3 = x2;
    gl_mul2w(x4, x2, x3, x);
    return gl_mul1w(x3, x4);
}
// two S-boxes at once: every product has an independent partner, no padding nops
__device__ __forceinline__ void sbox7x2(u64 &a, u64 &b) {
    u64 a2 = a, b2 = b;
    gl_mul2w(a2, a, b2, b);
    u64 a4 = a2, b4 = b2;
    gl_mul2w(a4, a2, b4, b2);
    gl_mul2w(a, a2, b, b2);        // a^3, b^3
    gl_mul2w(a, a4, b, b4);        // a^7, b^7
}

// default MDS (eigen_zeth_amd/poseidon_constants.py): circulant [17,15,41,16,2,28,13,13,39,18,34,20] + diag [8,0,..]
// coefficient of in[j] in out[i] is circ[(j-i) mod 12] (+8 at i=j=0).  As compile-time literals the
// entries are inline constants of v_mad_u64_u32: no SGPRs, no scalar loads.
__host__ __device__ __forceinline__ constexpr u32 def_mds(int i, int j) {
    constexpr u32 circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    return circ[(j - i + 12) % 12] + ((i == 0 && j == 0) ? 8u : 0u);
}

// s <- M*s + c   (c = the NEXT round's constants, or none): out[i] = sum_j m[i][j]*s[j] + c[i].
// m entries < 2^28 and s any u64: the two 64-bit partial sums over 32-bit halves cannot overflow
// (12 * 2^28 * 2^32 + 2^32 < 2^64).  Result weak.
// DEFMDS=false: injected matrix, staged once per workgroup in LDS (keeping 144 entries in SGPRs
// spills them to VGPR lanes; LDS reads of a wave-uniform address are broadcasts).
#include "poseidon_mds_asm.inc"   // mds_ark_default_asm: the default matrix as mad chains, 24 + 4 instructions per row

// the end of a row sum over any matrix with entries < 2^28: (alo, ahi) = the sums over the low and the high 32-bit halves, value = alo + ahi 2^32
// < 2^96  ->  weak.  Used by mds_ark's general branch, spread_perm and poseidon_trace_kernel
__device__ __forceinline__ u64 rowsum_reduce(u64 alo, u64 ahi) {
    const u64 mid = (alo >> 32) + ahi;  // value = (u32)alo + mid * 2^32
    return gl_reduce96_weak(((u64)(u32)mid << 32) | (u32)alo, (u32)(mid >> 32), 0u);
}

template <bool ADDC, bool DEFMDS>
__device__ __forceinline__ void mds_ark(u64 *s, const u32 *__restrict__ mds, const u64 *__restrict__ c) {
    if constexpr (DEFMDS) {
        mds_ark_default_asm<ADDC>(s, c);
        return;
    }
    u64 o[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        u64 alo = ADDC ? (u64)(u32)c[i] : 0ULL, ahi = ADDC ? (c[i] >> 32) : 0ULL;
        const u32 *mrow = mds + i * 12;  // DEFMDS=false: mds points at the workgroup's LDS copy
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const u32 m = DEFMDS ? def_mds(i, j) : mrow[j];
            alo += (u64)m * (u32)s[j];
            ahi += (u64)m * (u32)(s[j] >> 32);
        }
        o[i] = rowsum_reduce(alo, ahi);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = o[i];
}

// rows 0..3 of the default matrix product, no constants (the last round of a permutation whose caller reads a digest only)
__device__ __forceinline__ void mds_last4_default(u64 *s) {
    u32 lo[12], hi[12], o0[4], o1[4];
#pragma unroll
    for (int j = 0; j < 12; j++) { lo[j] = (u32)s[j]; hi[j] = (u32)(s[j] >> 32); }
    mds_rows_0_1(lo, hi, 0ULL, 0ULL, 0ULL, 0ULL, o0[0], o1[0], o0[1], o1[1]);
    mds_rows_2_3(lo, hi, 0ULL, 0ULL, 0ULL, 0ULL, o0[2], o1[2], o0[3], o1[3]);
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = ((u64)o1[j] << 32) | o0[j];
}

// ---- partial rounds THREE AT A TIME (default matrix; round 6).  A partial round is linear except for ONE S-box, so three of them are
// three S-boxes and ONE matrix product instead of three.  With t = the state after the first S-box (y0 in element 0), Z = "clear
// element 0", c1, c2, c3 the constants added after rounds r, r+1, r+2:
//     x1 = (M t)_0 + c1_0                                        y1 = x1^7
//     x2 = (M Z M t)_0 + M_00 y1 + (M Z c1 + c2)_0               y2 = x2^7
//     state entering round r+3 = (M Z)^2 M t + (M Z M e0) y1 + (M e0) y2 + [(M Z)^2 c1 + M Z c2 + c3]
// All matrices are products of M and M-with-column-0-cleared: non-negative integers below 2^21 (M^3 < 1 525 685), compile-time tables
// that the mads take from SGPRs; the three constant terms (14 words per block) are made on the host whenever a table is installed and sit
// behind the 360 round constants.  12 + 13 + 12 * 14 = 193 row terms per three rounds instead of 3 * 144: the 22 partial rounds cost
// 7 * (386 mads + 14 reductions) + one textbook round instead of 22 * (288 + 12).  The same field values as the textbook schedule
// (the oracle runs the textbook; every digest identical).  ZP_POSEIDON_BLOCK3=0 builds the textbook loop for A/B.
#ifndef ZP_POSEIDON_BLOCK3
#define ZP_POSEIDON_BLOCK3 1
#endif
#define ZP_POSEIDON_PK_BLOCKS 7          // partial rounds 4..24 in blocks of three; round 25 stays textbook
#define ZP_POSEIDON_PK_WORDS 14          // k1, k2, K3[12]
struct P3Tab {
    u32 r1[12];       // row 0 of M
    u32 r2[12];       // row 0 of M Z M
    u32 a3[12][12];   // (M Z)^2 M
    u32 u[12];        // column 0 of M Z M
    u32 v[12];        // column 0 of M
    u32 mz[12][12];   // M Z (host: the constant terms)
};
__host__ __device__ constexpr P3Tab p3_tab() {
    P3Tab t{};
    u32 m[12][12] = {}, mz[12][12] = {}, a2[12][12] = {};
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) {
            m[i][j] = def_mds(i, j);
            mz[i][j] = j == 0 ? 0u : def_mds(i, j);
        }
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) {
            u32 acc = 0;
            for (int k = 0; k < 12; k++) acc += mz[i][k] * m[k][j];
            a2[i][j] = acc;
        }
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) {
            u32 acc = 0;
            for (int k = 0; k < 12; k++) acc += mz[i][k] * a2[k][j];
            t.a3[i][j] = acc;
            t.mz[i][j] = mz[i][j];
        }
    for (int j = 0; j < 12; j++) {
        t.r1[j] = m[0][j];
        t.r2[j] = a2[0][j];
        t.u[j] = a2[j][0];
        t.v[j] = m[j][0];
    }
    return t;
}
// alo + ahi 2^32, both < 2^58  ->  weak.  The tail of poseidon_mds_asm.inc's rows: T = alo + (ahi >> 32) EPS (no overflow: < 2^59), then
// hi(T) + lo(ahi) with 2^64 == EPS folded back (carry c: lo -= 1, and hi += 1 unless that borrowed) -- four VALU instructions
__device__ __forceinline__ u64 p3_reduce(u64 alo, u64 ahi) {
    const u64 t = (u64)(u32)(ahi >> 32) * 0xFFFFFFFFu + alo;
    const u32 tl = (u32)t, th = (u32)(t >> 32), b0 = (u32)ahi;
    u32 r0, r1;
    u64 c, d;
    asm("v_add_co_u32 %1, %2, %5, %6\n\t"
        "s_nop 0\n\t"
        "v_subbrev_co_u32 %0, %3, 0, %4, %2\n\t"
        "s_nop 0\n\t"
        "s_andn2_b64 %2, %2, %3\n\t"
        "v_addc_co_u32 %1, %3, %1, 0, %2"
        : "=&v"(r0), "=&v"(r1), "=&s"(c), "=&s"(d)
        : "v"(tl), "v"(th), "v"(b0)
        : "scc");
    return ((u64)r1 << 32) | r0;
}
// s: the state entering partial round r (its constants added); pk: the block's 14 constant words.  Leaves the state entering round r + 3.
__device__ __forceinline__ void partial3_default(u64 *s, const u64 *__restrict__ pk) {
    constexpr P3Tab T = p3_tab();
    s[0] = sbox7(s[0]);
    u32 lo[12], hi[12];
#pragma unroll
    for (int j = 0; j < 12; j++) { lo[j] = (u32)s[j]; hi[j] = (u32)(s[j] >> 32); }
    u64 alo = (u64)(u32)pk[0], ahi = pk[0] >> 32;
#pragma unroll
    for (int j = 0; j < 12; j++) { alo += (u64)T.r1[j] * lo[j]; ahi += (u64)T.r1[j] * hi[j]; }
    const u64 y1 = sbox7(p3_reduce(alo, ahi));
    const u32 y1l = (u32)y1, y1h = (u32)(y1 >> 32);
    alo = (u64)(u32)pk[1];
    ahi = pk[1] >> 32;
#pragma unroll
    for (int j = 0; j < 12; j++) { alo += (u64)T.r2[j] * lo[j]; ahi += (u64)T.r2[j] * hi[j]; }
    alo += (u64)T.v[0] * y1l;
    ahi += (u64)T.v[0] * y1h;
    const u64 y2 = sbox7(p3_reduce(alo, ahi));
    const u32 y2l = (u32)y2, y2h = (u32)(y2 >> 32);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        alo = (u64)(u32)pk[2 + i];
        ahi = pk[2 + i] >> 32;
#pragma unroll
        for (int j = 0; j < 12; j++) { alo += (u64)T.a3[i][j] * lo[j]; ahi += (u64)T.a3[i][j] * hi[j]; }
        alo += (u64)T.u[i] * y1l;
        ahi += (u64)T.u[i] * y1h;
        alo += (u64)T.v[i] * y2l;
        ahi += (u64)T.v[i] * y2h;
        s[i] = p3_reduce(alo, ahi);
    }
}

// textbook schedule ARK -> S-box -> MDS, with each round's ARK folded into the previous round's
// MDS accumulators; state is weak between rounds and canonicalised once at the end.
// OUT4: the caller reads s[0..4) alone (a digest: Merkle leaves and nodes, the grinding hash) -- four rows of the last matrix product
// instead of twelve; s[4..12) are left stale
template <bool DEFMDS, bool OUT4 = false>
__device__ __forceinline__ void poseidon_perm(u64 *s, const u64 *__restrict__ rc, const u32 *__restrict__ mds) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_weak(s[i], rc[i]);
    if constexpr (DEFMDS && ZP_POSEIDON_BLOCK3) {
#pragma unroll 1
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int i = 0; i < 12; i += 2) sbox7x2(s[i], s[i + 1]);
            mds_ark<true, true>(s, mds, rc + (r + 1) * 12);
        }
#pragma unroll 1
        for (int b = 0; b < ZP_POSEIDON_PK_BLOCKS; b++) partial3_default(s, rc + 360 + b * ZP_POSEIDON_PK_WORDS);
        s[0] = sbox7(s[0]);                                   // round 25
        mds_ark<true, true>(s, mds, rc + 26 * 12);
#pragma unroll 1
        for (int r = 26; r < 29; r++) {
#pragma unroll
            for (int i = 0; i < 12; i += 2) sbox7x2(s[i], s[i + 1]);
            mds_ark<true, true>(s, mds, rc + (r + 1) * 12);
        }
#pragma unroll
        for (int i = 0; i < 12; i += 2) sbox7x2(s[i], s[i + 1]);
        if constexpr (OUT4) {
            mds_last4_default(s);
#pragma unroll
            for (int i = 0; i < 4; i++) s[i] = gl_canon(s[i]);
        } else {
            mds_ark<false, true>(s, mds, rc);
#pragma unroll
            for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
        }
        return;
    }
#pragma unroll 1
    for (int r = 0; r < 29; r++) {
        if (r < 4 || r >= 26) {
#pragma unroll
            for (int i = 0; i < 12; i += 2) sbox7x2(s[i], s[i + 1]);
        } else {
            s[0] = sbox7(s[0]);
        }
        mds_ark<true, DEFMDS>(s, mds, rc + (r + 1) * 12);
    }
#pragma unroll
    for (int i = 0; i < 12; i += 2) sbox7x2(s[i], s[i + 1]);
    mds_ark<false, DEFMDS>(s, mds, rc);
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
}

template <bool DEFMDS>
__device__ __forceinline__ const u32 *stage_mds(const u32 *mds, u32 *smds) {
    if constexpr (DEFMDS) {
        return mds;
    } else {
        if (threadIdx.x < 144) smds[threadIdx.x] = mds[threadIdx.x];
        __syncthreads();
        return smds;
    }
}

template <bool DEFMDS>
__global__ void __launch_bounds__(256) poseidon_perm_kernel(u64 *states, size_t count, const u64 *rc, const u32 *mds) {
    __shared__ u32 smds[DEFMDS ? 1 : 144];
    mds = stage_mds<DEFMDS>(mds, smds);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    u64 s[12];
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = states[i * 12 + j];
    poseidon_perm<DEFMDS>(s, rc, mds);
#pragma unroll
    for (int j = 0; j < 12; j++) states[i * 12 + j] = s[j];
}

// ---- the SPREAD-STATE permutation: one lane per state WORD instead of one lane per state.  12 lanes share a permutation through a 12-word LDS
// row, so a round is one S-box + one 12-term row sum per lane (~150 dependent instructions) instead of ~1600 on a single lane: the latency form,
// for everything that has fewer permutations in flight than the chip has lanes.  Lane e holds word e; per round it adds its constant, applies x^7
// (full rounds, or word 0), publishes its word, sums its matrix row over the 12 published words in two 32-bit halves and reduces.  Textbook
// schedule; canonical out.
//   sh: the lane's row of the exchange buffer;  rc: the 360 round constants ALREADY OFFSET to the lane's word (global memory or an LDS copy);
//   m: the lane's 12 matrix coefficients (global mds + 12 e, or registers);  on: guards the LDS write and the row sum -- a lane that is off runs
//   both barriers of every round, never touches sh (its row may lie past the buffer) and returns garbage.
// Callers: poseidon_perm_small_kernel, wave12_perm (the single-wave kernels), merkle_leaves_coop_kernel, merkle_subtree_kernel.
__device__ __forceinline__ u64 spread_perm(u64 s, int e, bool on, u64 *sh, const u64 *rc, const u32 *m) {
    for (int r = 0; r < 30; r++) {
        s = gl_add_weak(s, rc[r * 12]);
        if (r < 4 || r >= 26 || e == 0) s = sbox7(s);
        if (on) sh[e] = s;
        __syncthreads();
        u64 alo = 0, ahi = 0;
        if (on) {
#pragma unroll
            for (int j = 0; j < 12; j++) {
                const u64 v = sh[j];
                alo += (u64)m[j] * (u32)v;
                ahi += (u64)m[j] * (u32)(v >> 32);
            }
        }
        __syncthreads();
        s = rowsum_reduce(alo, ahi);
    }
    return gl_canon(s);
}

// A handful of permutations (count <= 64: a transcript state at a time): five states per wave, lanes 60..63 idle (q = 5 is past the buffer)
__global__ void __launch_bounds__(64) poseidon_perm_small_kernel(u64 *states, int count, const u64 *rc, const u32 *mds) {
    __shared__ u64 sh[5][12];
    const int lane = threadIdx.x, q = lane / 12, e = lane % 12;
    const int perm = blockIdx.x * 5 + q;
    const bool on = q < 5 && perm < count;
    u64 s = on ? states[(size_t)perm * 12 + e] : 0ULL;
    s = spread_perm(s, e, on, sh[q], rc + e, mds + e * 12);
    if (on) states[(size_t)perm * 12 + e] = s;
}

// one permutation of the state a wave holds in its lanes 0..11 (the single-wave kernels: transcript steps, recursion-witness walks)
// (the round constants come from LDS -- rcs: all 360, loaded once per kernel by wave12_tables -- and the lane's matrix row from registers: a
// permutation of these single-wave kernels is a chain of 30 dependent rounds, and a global load of a constant sat in every link)
__device__ __forceinline__ void wave12_tables(int e, bool on, const u64 *rc, const u32 *mds, u64 *rcs, u32 *row) {
    for (int i = threadIdx.x; i < 360; i += 64) rcs[i] = rc[i];
#pragma unroll
    for (int j = 0; j < 12; j++) row[j] = mds[(on ? e : 0) * 12 + j];
    __syncthreads();
}
__device__ __forceinline__ u64 wave12_perm(u64 s, int e, bool on, u64 *sh, const u64 *rcs, const u32 *row) {
    return spread_perm(s, e, on, sh, rcs + (on ? e : 0), row);
}

// The Fiat-Shamir sponge as ONE launch: buf = [12 state words][nblocks x 8 block words][(1 + extra) x 8 rate words out][caps out].
// For every block: the rate (state[0..8)) is overwritten with the block, then one permutation (no block: one permutation);
// then `extra` further permutations, the rate after each of the 1 + extra steps is written out.  Same 12-lanes-per-state form
// as above: a transcript of k permutations costs one host round trip instead of k.
// caps (want_caps): the capacity (state[8..12)) after EVERY permutation, 4 words each -- with the blocks and the rates that is the
// input state of every permutation of the step, what the verifier AIR's witness needs (stark/verifier_air.py: transcript blocks).
//
// STAGED: the buffer is PAGE-LOCKED, device-visible host memory (round 5): the host writes state and blocks into the ctx's staging buffer, the kernel
// pulls them into LDS in one coalesced sweep, walks them, and posts state, rates and capacities straight back -- one launch and two stream
// synchronisations per transcript step instead of four launches (copy kernels in and out) and four synchronisations: a step went from ~180 us to
// ~45 us, and a proof has 9-12 of them, a recursion witness ~24.  Not STAGED (an input above 48 KiB): buf is device memory, read in place.
template <bool STAGED>
__global__ void __launch_bounds__(64) poseidon_sponge_kernel(u64 *buf, int nblocks, int extra, const u64 *rc, const u32 *mds, int want_caps) {
    extern __shared__ u64 stage[];              // STAGED: [12 + nblocks * 8]
    __shared__ u64 sh[12];
    __shared__ u64 rcs[360];
    const int e = threadIdx.x;
    const bool on = e < 12;
    u32 row[12];
    wave12_tables(e, on, rc, mds, rcs, row);
    const int nin = 12 + nblocks * 8;
    if constexpr (STAGED) {
        for (int i = e; i < nin; i += 64) stage[i] = buf[i];
        __syncthreads();
    }
    const u64 *in = STAGED ? stage : buf;
    u64 s = on ? in[e] : 0ULL;
    u64 *rates = buf + nin, *caps = rates + (size_t)(1 + extra) * 8;
    const int absorb = nblocks > 0 ? nblocks : 1;
    for (int b = 0; b < absorb + extra; b++) {
        if (b < nblocks && e < 8) s = in[12 + b * 8 + e];
        s = wave12_perm(s, e, on, sh, rcs, row);
        if (b >= absorb - 1 && e < 8) rates[(size_t)(b - (absorb - 1)) * 8 + e] = s;
        if (want_caps && on && e >= 8) caps[(size_t)b * 4 + (e - 8)] = s;
    }
    if (on) buf[e] = s;
}

// ---- the hashing walk of a recursion witness on the device (csrc/recursion.hip, round 5): no host round trip per permutation
// Whole Fiat-Shamir transcripts in ONE launch: workgroup c walks the steps [first[c], first[c + 1]) of chain c from the zero state; a step
// overwrites the rate with its block (absorb[s] != 0) or just permutes; out[s] = the 12 words entering the permutation, then the rate after it
__global__ void __launch_bounds__(64) sponge_chains_kernel(const u64 *__restrict__ blocks, const unsigned char *__restrict__ absorb,
                                                           const unsigned int *__restrict__ first, u64 *__restrict__ out, const u64 *rc, const u32 *mds) {
    __shared__ u64 sh[12];
    __shared__ u64 rcs[360];
    const int e = threadIdx.x;
    const bool on = e < 12;
    u32 row[12];
    wave12_tables(e, on, rc, mds, rcs, row);
    u64 s = 0;
    for (unsigned int st = first[blockIdx.x]; st < first[blockIdx.x + 1]; st++) {
        if (absorb[st] && e < 8) s = blocks[(size_t)st * 8 + e];
        if (on) out[(size_t)st * 20 + e] = s;
        s = wave12_perm(s, e, on, sh, rcs, row);
        if (e < 8) out[(size_t)st * 20 + 12 + e] = s;
    }
}

// Every opening of a recursion witness in ONE launch: workgroup o hashes the leaf of opening o (na blocks of 8 values: the linear hash of
// merkle_leaves_kernel -- words 0..3 of a permutation's output are the capacity of the next block) and walks its nd path levels along the bits
// of its index; the 12 words entering every permutation go to inputs[b0 + ...] (the verifier AIR's permutation blocks, in HBM where
// zp_poseidon_trace reads them), the last digest to digests[o].   op: b0, na, nd per opening; vals: mw words per opening, zero padded;
// sib: the siblings of opening o at sib_off[o], 4 words per level
__global__ void __launch_bounds__(64) openings_walk_kernel(const u64 *__restrict__ op, const u64 *__restrict__ vals, u64 mw, const u64 *__restrict__ index,
                                                           const u64 *__restrict__ sib, const u64 *__restrict__ sib_off, u64 *__restrict__ inputs,
                                                           u64 *__restrict__ digests, const u64 *rc, const u32 *mds) {
    __shared__ u64 sh[12];
    __shared__ u64 cur[4];
    __shared__ u64 rcs[360];
    const int e = threadIdx.x;
    const bool on = e < 12;
    u32 row[12];
    wave12_tables(e, on, rc, mds, rcs, row);
    const u64 o = blockIdx.x, b0 = op[3 * o], na = op[3 * o + 1], nd = op[3 * o + 2];
    const u64 *v = vals + o * mw;
    u64 s = 0;
    if (e < 4) cur[e] = v[e];                               // an unhashed leaf (<= 4 values) is its own digest, zero padded
    for (u64 j = 0; j < na; j++) {
        if (e < 8) s = 8 * j + e < mw ? v[8 * j + e] : 0ULL;
        if (on) inputs[(b0 + j) * 12 + e] = s;
        s = wave12_perm(s, e, on, sh, rcs, row);
        if (on) sh[e] = s;
        __syncthreads();
        if (e >= 8 && on) s = sh[e - 8];                    // the digest so far is the next block's capacity
        if (e < 4) cur[e] = s;
        __syncthreads();
    }
    const u64 idx = index[o];
    const u64 *sb = sib + sib_off[o];
    __syncthreads();
    for (u64 lv = 0; lv < nd; lv++) {
        const bool bit = (idx >> lv) & 1;
        if (on) {
            if (e < 4) s = bit ? sb[lv * 4 + e] : cur[e];
            else if (e < 8) s = bit ? cur[e - 4] : sb[lv * 4 + (e - 4)];
            else s = 0;
            inputs[(b0 + na + lv) * 12 + e] = s;
        }
        __syncthreads();
        s = wave12_perm(s, e, on, sh, rcs, row);
        if (e < 4) cur[e] = s;
        __syncthreads();
    }
    if (e < 4) digests[o * 4 + e] = cur[e];
}

// ---- a verifier's openings, throughput form: ONE LANE PER OPENING, the state in registers.  A lane absorbs its leaf in blocks of 8 with the digest
// so far as the next capacity (merkle_leaves_kernel's linear hash; <= 4 values are their own digest, zero padded), then hashes `depth` nodes
// along the bits of its index and compares with its root: one flag per opening.  Openings of one launch come from trees of different width and
// depth; the host sorts them into SEGMENTS of one (width, depth) each and packs a segment word-major -- word k of its opening i at
// vals[voff + k n + i], word w of the sibling of level l at sibs[soff + (4 l + w) n + i] -- so that the lanes of a wave read consecutive
// words.  A wave runs as many steps as its longest lane needs; a lane past its own count keeps its digest (predicated, no early exit).
struct VerifySeg { u64 voff, soff; u32 o0, n, width, depth; };
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
template <bool DEFMDS>
__global__ void __launch_bounds__(256) openings_lane_kernel(const VerifySeg *__restrict__ segs, const u32 *__restrict__ seg_of, const u32 *__restrict__ root_slot,
                                                           const u64 *__restrict__ index, const u64 *__restrict__ roots, const u64 *__restrict__ vals,
                                                           const u64 *__restrict__ sibs, size_t count, unsigned char *__restrict__ ok, const u64 *rc,
                                                           const u32 *mds) {
    __shared__ u32 smds[DEFMDS ? 1 : 144];
    mds = stage_mds<DEFMDS>(mds, smds);
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = o < count;
    VerifySeg sg = {0, 0, 0, 1, 0, 0};
    if (live) sg = segs[seg_of[o]];
    const size_t i = live ? o - sg.o0 : 0;
    const int nblk = sg.width > 4 ? (int)((sg.width + 7) / 8) : 0, nsteps = live ? nblk + (int)sg.depth : 0;
    const u64 idx = live ? index[o] : 0;
    u64 cur[4];
#pragma unroll
    for (int j = 0; j < 4; j++) cur[j] = (live && sg.width <= 4 && (u32)j < sg.width) ? vals[sg.voff + (size_t)j * sg.n + i] : 0ULL;
    const int wsteps = wave_max_i32(nsteps);
#pragma unroll 1
    for (int st = 0; st < wsteps; st++) {
        const bool on = st < nsteps, leaf = st < nblk;
        u64 s[12];
        const bool bit = on && !leaf && ((idx >> (st - nblk)) & 1);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // a leaf step reads values 8 st + j and 8 st + 4 + j, a node step word j of the level's sibling
            const u32 k = 8u * (u32)st + (u32)j;
            const u64 a = !on ? 0ULL : leaf ? (k < sg.width ? vals[sg.voff + (size_t)k * sg.n + i] : 0ULL) : sibs[sg.soff + (size_t)(4 * (st - nblk) + j) * sg.n + i];
            const u64 b = (on && leaf && k + 4 < sg.width) ? vals[sg.voff + (size_t)(k + 4) * sg.n + i] : 0ULL;
            s[j] = (leaf || bit) ? a : cur[j];
            s[4 + j] = leaf ? b : (bit ? cur[j] : a);
            s[8 + j] = leaf ? cur[j] : 0ULL;           // the digest so far is the next block's capacity (zero before the first)
        }
        poseidon_perm<DEFMDS, true>(s, rc, mds);
#pragma unroll
        for (int j = 0; j < 4; j++) cur[j] = on ? s[j] : cur[j];
    }
    if (live) {
        const u64 *r = roots + 4 * (size_t)root_slot[o];
        ok[o] = (cur[0] == r[0] && cur[1] == r[1] && cur[2] == r[2] && cur[3] == r[3]) ? 1 : 0;
    }
}

// proof-of-work grinding (before the query phase of a STARK): lane = candidate nonce base + gid; a hit is a nonce with
// Poseidon(seed[0..3] || nonce || 0^7)[0] >> (64 - bits) == 0; the smallest hit of the batch wins (atomicMin).
template <bool DEFMDS>
__global__ void __launch_bounds__(256) pow_grind_kernel(const u64 *__restrict__ seed4, int bits, u64 base, u64 *best,
                                                       const u64 *rc, const u32 *mds) {
    __shared__ u32 smds[DEFMDS ? 1 : 144];
    mds = stage_mds<DEFMDS>(mds, smds);
    const u64 nonce = base + (u64)blockIdx.x * 256 + threadIdx.x;
    u64 s[12];
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = seed4[j];
    s[4] = nonce;
#pragma unroll
    for (int j = 5; j < 12; j++) s[j] = 0;
    poseidon_perm<DEFMDS, true>(s, rc, mds);
    if ((s[0] >> (64 - bits)) == 0) atomicMin((unsigned long long *)best, (unsigned long long)nonce);
}

// Round-by-round trace of permutations: the witness of a Poseidon AIR (stark/verifier_air.py).  lane = permutation k, block of 32
// rows: states[e][32 k + r] = element e of the state BEFORE round r (r < 30), the output on rows 30 and 31;
// cubes[e][32 k + r] = (state + round constant)^3 (rows 30, 31: state^3) -- the helper column that keeps x^7 at degree 3.
// Canonical values throughout (they are committed).  Column stride in elements.
__global__ void __launch_bounds__(128) poseidon_trace_kernel(const u64 *__restrict__ inputs, size_t count, u64 *__restrict__ states,
                                                            u64 *__restrict__ cubes, size_t stride, const u64 *__restrict__ rc,
                                                            const u32 *__restrict__ mds) {
    __shared__ u32 smds[144];
    if (threadIdx.x < 144 - 128) smds[128 + threadIdx.x] = mds[128 + threadIdx.x];
    smds[threadIdx.x] = mds[threadIdx.x];
    __syncthreads();
    const size_t k = (size_t)blockIdx.x * 128 + threadIdx.x;
    if (k >= count) return;
    u64 s[12];
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = inputs[k * 12 + j];
    const size_t row0 = 32 * k;
#pragma unroll 1
    for (int r = 0; r < 32; r++) {
        const bool round = r < 30;
        const bool full = r < 4 || r >= 26;
        u64 y[12];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const u64 x = round ? gl_add(s[j], rc[r * 12 + j]) : s[j];
            const u64 c = gl_mul(gl_mul(x, x), x);
            states[(size_t)j * stride + row0 + r] = s[j];
            cubes[(size_t)j * stride + row0 + r] = c;
            y[j] = (full || j == 0) ? gl_mul(gl_mul(c, c), x) : x;
        }
        if (!round) continue;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            u64 alo = 0, ahi = 0;
#pragma unroll
            for (int j = 0; j < 12; j++) {
                const u32 m = smds[i * 12 + j];
                alo += (u64)m * (u32)y[j];
                ahi += (u64)m * (u32)(y[j] >> 32);
            }
            s[i] = gl_canon(rowsum_reduce(alo, ahi));
        }
    }
}

// leaf i = linear hash of its `len` values: blocks of 8 into the rate, the digest so far as the next capacity (<= 4 values are their own digest,
// zero padded);  lane = leaf, the throughput form.  ROWS = false: `len` columns of M values (value k of leaf i at src[k M + i]; every column
// read is a coalesced 512-byte run per wave);  ROWS = true: M contiguous rows of `len` values (src[i len + k])
template <bool ROWS> using leaf_len_t = std::conditional_t<ROWS, size_t, int>;      // as the C ABI gives it: zp_merkle_commit's W is an int32
template <bool DEFMDS, bool ROWS>
__global__ void __launch_bounds__(256) merkle_leaves_kernel(const u64 *__restrict__ src, size_t M, leaf_len_t<ROWS> len,
                                                           u64 *__restrict__ tree, const u64 *rc, const u32 *mds) {
    __shared__ u32 smds[DEFMDS ? 1 : 144];
    mds = stage_mds<DEFMDS>(mds, smds);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const u64 *row = src + i * (size_t)len;      // ROWS
    auto at = [&](leaf_len_t<ROWS> k) { return k < len ? (ROWS ? row[k] : src[(size_t)k * M + i]) : 0ULL; };     // value k of leaf i, zero past the end
    u64 s[12];
    if (len <= 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) tree[i * 4 + j] = at(j);
        return;
    }
#pragma unroll
    for (int j = 8; j < 12; j++) s[j] = 0;
    for (leaf_len_t<ROWS> off = 0; off < len; off += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = at(off + j);
        poseidon_perm<DEFMDS, true>(s, rc, mds);
#pragma unroll
        for (int j = 0; j < 4; j++) s[8 + j] = s[j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) tree[i * 4 + j] = s[8 + j];
}

// Small trees (FRI layers below 2^14 leaves): 12 lanes per leaf, like merkle_subtree_kernel -- a leaf of 24 values is
// three dependent permutations, 0.33 ms on a single lane while the chip idles, ~50 us with the state spread over lanes.
// 64 leaves per workgroup, lane = (leaf, element), one spread_perm row each; constants and matrix row from global memory (L2: 768 lanes share them).
// stride_e / stride_i: element (row i, position k) sits at src[k * stride_e + i * stride_i]  (columns: M, 1; rows: 1, len)
__global__ void __launch_bounds__(768) merkle_leaves_coop_kernel(const u64 *__restrict__ src, size_t M, size_t len, size_t stride_e,
                                                                size_t stride_i, u64 *__restrict__ tree, const u64 *rc,
                                                                const u32 *mds) {
    __shared__ u64 sh[64][12];
    const int node = threadIdx.x / 12, e = threadIdx.x % 12;
    const size_t i = (size_t)blockIdx.x * 64 + node;
    const bool on = i < M;                       // every lane runs the barriers; idle leaves compute on zeros
    if (len <= 4) {
        if (on && e < 4) tree[i * 4 + e] = (size_t)e < len ? src[(size_t)e * stride_e + i * stride_i] : 0ULL;
        return;
    }
    u64 s = 0;
    for (size_t off = 0; off < len; off += 8) {
        if (e < 8) s = (on && off + e < len) ? src[(off + e) * stride_e + i * stride_i] : 0ULL;
        s = spread_perm(s, e, true, sh[node], rc + e, mds + e * 12);
        // capacity of the next block = the first four outputs
        sh[node][e] = s;
        __syncthreads();
        const u64 cap = sh[node][e & 3];
        __syncthreads();
        if (e >= 8) s = cap;
        else if (off + 8 >= len && e < 4 && on) tree[i * 4 + e] = s;
    }
}

// one tree level: node i = P(child[2i] || child[2i+1] || 0^4)[0..4]
template <bool DEFMDS>
__global__ void __launch_bounds__(256) merkle_level_kernel(const u64 *__restrict__ prev, u64 *__restrict__ next,
                                                          size_t half, const u64 *rc, const u32 *mds) {
    __shared__ u32 smds[DEFMDS ? 1 : 144];
    mds = stage_mds<DEFMDS>(mds, smds);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= half) return;
    u64 s[12];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = prev[i * 8 + j];
#pragma unroll
    for (int j = 8; j < 12; j++) s[j] = 0;
    poseidon_perm<DEFMDS, true>(s, rc, mds);
#pragma unroll
    for (int j = 0; j < 4; j++) next[i * 4 + j] = s[j];
}

// upper part of the tree, up to 7 levels per launch, 12 lanes per node: workgroup b reduces nodes
// [128b, 128b+128) of the level at `prev` (cnt nodes, a power of two) through nlev levels.  The lane-per-node kernel
// below ~2^15 nodes is latency-bound (one permutation takes a single lane ~0.1 ms); spreading a state over 12 lanes
// brings a level to ~30 us, and fusing the levels of a 128-node subtree removes the launches in between.
__global__ void __launch_bounds__(768) merkle_subtree_kernel(u64 *prev, size_t cnt, int nlev, const u64 *rc, const u32 *mds) {
    __shared__ u64 sh[64][12];
    const int node = threadIdx.x / 12, e = threadIdx.x % 12;
    size_t first = (size_t)blockIdx.x * 128;          // first node of this workgroup in the current level
    size_t width = cnt < 128 ? cnt : 128;             // nodes of the current level this workgroup owns
    for (int l = 0; l < nlev; l++) {
        const size_t half = width >> 1;
        u64 *next = prev + cnt * 4;
        const bool on = (size_t)node < half;
        u64 s = (on && e < 8) ? prev[(first + 2 * (size_t)node) * 4 + e] : 0ULL;
        s = spread_perm(s, e, true, sh[node], rc + e, mds + e * 12);     // idle nodes hash zeros in rows of their own
        if (on && e < 4) next[((first >> 1) + (size_t)node) * 4 + e] = s;
        __threadfence_block();
        __syncthreads();
        prev = next;
        cnt >>= 1;
        first >>= 1;
        width = half;
    }
}

// the one place that turns ctx->mds_is_default into a template argument: kt / kf are the <true> / <false> instantiations of one throughput
// kernel (256 lanes per workgroup, a parameter list that ends ..., rc, mds)
template <class K, class... A>
void launch_mds(zp_ctx *ctx, K kt, K kf, size_t blocks, A... args) {
    hipLaunchKernelGGL(ctx->mds_is_default ? kt : kf, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, args..., ctx->d_rc, ctx->d_mds);
}

int32_t tree_levels(zp_ctx *ctx, u64 *tree, size_t M) {
    u64 *prev = tree;
    size_t cnt = M;
    while (cnt > 1) {
        u64 *next = prev + cnt * 4;
        const size_t half = cnt >> 1;
        if (cnt <= ((size_t)1 << (ctx->tune_merkle_coop_log > 0 ? ctx->tune_merkle_coop_log : 15))) {
            int lg = 0;
            while (((size_t)1 << lg) < cnt) lg++;
            const int nlev = lg < 7 ? lg : 7;
            hipLaunchKernelGGL(merkle_subtree_kernel, dim3((unsigned)(cnt < 128 ? 1 : cnt / 128)), dim3(768), 0, ctx->stream,
                               prev, cnt, nlev, ctx->d_rc, ctx->d_mds);
            ZP_HIP(ctx, hipGetLastError());
            for (int l = 0; l < nlev; l++) {
                prev += cnt * 4;
                cnt >>= 1;
            }
            continue;
        }
        launch_mds(ctx, merkle_level_kernel<true>, merkle_level_kernel<false>, (half + 255) / 256, (const u64 *)prev, next, half);
        ZP_HIP(ctx, hipGetLastError());
        prev = next;
        cnt = half;
    }
    return ZP_OK;
}

// leaves and levels of one tree: M leaves of `len` values, as columns (ROWS = false) or as rows.  Trees of <= 2^14 hashed leaves take the
// 12-lanes-per-leaf kernel, everything else one lane per leaf
template <bool ROWS>
int32_t commit_tree(zp_ctx *ctx, const u64 *src, size_t M, size_t len, u64 *tree) {
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    if (M <= ((size_t)1 << 14) && len > 4)
        hipLaunchKernelGGL(merkle_leaves_coop_kernel, dim3((unsigned)((M + 63) / 64)), dim3(768), 0, ctx->stream, src, M, len,
                           ROWS ? (size_t)1 : M, ROWS ? len : (size_t)1, tree, ctx->d_rc, ctx->d_mds);
    else
        launch_mds(ctx, merkle_leaves_kernel<true, ROWS>, merkle_leaves_kernel<false, ROWS>, (M + 255) / 256, src, M, (leaf_len_t<ROWS>)len, tree);
    ZP_HIP(ctx, hipGetLastError());
    return tree_levels(ctx, tree, M);
}

}  // namespace

int32_t zpi_poseidon_sync_tables(zp_ctx *ctx) {
    if (!ctx->poseidon_dirty) return ZP_OK;
    for (int i = 0; i < 144; i++) ZP_ARG(ctx, ctx->h_mds[i] < (1ULL << 28), "MDS entries must be < 2^28");
    if (!ctx->d_rc) ZP_HIP(ctx, hipMalloc((void **)&ctx->d_rc, (360 + ZP_POSEIDON_PK_BLOCKS * ZP_POSEIDON_PK_WORDS) * sizeof(u64)));
    if (!ctx->d_mds) ZP_HIP(ctx, hipMalloc((void **)&ctx->d_mds, 144 * sizeof(u32)));
    u32 m32[144];
    for (int i = 0; i < 144; i++) m32[i] = (u32)ctx->h_mds[i];
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ZP_HIP(ctx, hipMemcpy(ctx->d_rc, ctx->h_rc, 360 * sizeof(u64), hipMemcpyHostToDevice));
    ZP_HIP(ctx, hipMemcpy(ctx->d_mds, m32, sizeof(m32), hipMemcpyHostToDevice));
    ctx->mds_is_default = true;
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++)
            if (ctx->h_mds[i * 12 + j] != def_mds(i, j)) ctx->mds_is_default = false;
    if (ctx->mds_is_default) {
        // constant terms of the three-round blocks (partial3_default): k1 = c1_0, k2 = (M Z c1 + c2)_0, K3 = (M Z)^2 c1 + M Z c2 + c3
        constexpr P3Tab T = p3_tab();
        u64 pk[ZP_POSEIDON_PK_BLOCKS * ZP_POSEIDON_PK_WORDS];
        auto mzv = [&](const u64 *x, u64 *y) {
            for (int i = 0; i < 12; i++) {
                u64 acc = 0;
                for (int j = 1; j < 12; j++) acc = gl_add(acc, gl_mul((u64)T.mz[i][j], x[j]));
                y[i] = acc;
            }
        };
        for (int b = 0; b < ZP_POSEIDON_PK_BLOCKS; b++) {
            const int r = 4 + 3 * b;
            const u64 *c1 = ctx->h_rc + (r + 1) * 12, *c2 = ctx->h_rc + (r + 2) * 12, *c3 = ctx->h_rc + (r + 3) * 12;
            u64 t1[12], t2[12], t3[12];
            mzv(c1, t1);                 // M Z c1
            mzv(t1, t2);                 // (M Z)^2 c1
            mzv(c2, t3);                 // M Z c2
            u64 *o = pk + b * ZP_POSEIDON_PK_WORDS;
            o[0] = gl_canon(c1[0]);
            o[1] = gl_add(t1[0], gl_canon(c2[0]));
            for (int i = 0; i < 12; i++) o[2 + i] = gl_add(gl_add(t2[i], t3[i]), gl_canon(c3[i]));
        }
        ZP_HIP(ctx, hipMemcpy(ctx->d_rc + 360, pk, sizeof(pk), hipMemcpyHostToDevice));
    }
    ctx->poseidon_dirty = false;
    return ZP_OK;
}

// nsteps steps of nchains sponge chains in one launch (sponge_chains_kernel); d_*: device buffers the caller filled, d_out u64[nsteps][20]
int32_t zpi_poseidon_chains(zp_ctx *ctx, const u64 *d_blocks, const unsigned char *d_absorb, const unsigned int *d_first, int nchains, u64 *d_out) {
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    if (nchains <= 0) return ZP_OK;
    hipLaunchKernelGGL(sponge_chains_kernel, dim3((unsigned)nchains), dim3(64), 0, ctx->stream, d_blocks, d_absorb, d_first, d_out, ctx->d_rc, ctx->d_mds);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

// the same from host buffers, for a verifier's transcripts (csrc/verify.hip): h_blocks u64[nsteps][8], h_rates u64[nsteps][8] = the rate after every
// step.  [blocks][out, 20 words per step][first][absorb] in one device buffer; one upload, one launch, one download, one synchronisation
int32_t zpi_poseidon_chains_host(zp_ctx *ctx, const u64 *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int nchains, u64 *h_rates) {
    ZP_BIND(ctx);
    ZP_ARG(ctx, nchains > 0 && h_blocks && h_absorb && h_first && h_rates && h_first[nchains] > 0, "bad chains");
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    const size_t nsteps = h_first[nchains], o_out = 8 * nsteps, o_first = o_out + 20 * nsteps, o_abs = o_first + ((size_t)nchains + 2) / 2, total = o_abs + (nsteps + 7) / 8;
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (an earlier small copy may still read the staging buffer)
    void *stv = nullptr;
    ZP_TRY(zpi_pinned(ctx, total * 8, &stv));
    u64 *buf = (u64 *)stv, *dbuf = nullptr;
    memcpy(buf, h_blocks, 64 * nsteps);
    memcpy(buf + o_first, h_first, 4 * ((size_t)nchains + 1));
    memcpy(buf + o_abs, h_absorb, nsteps);
    ZP_TRY(zpi_scratch(ctx, 3, total, &dbuf));
    ZP_HIP(ctx, hipMemcpyAsync(dbuf, buf, 64 * nsteps, hipMemcpyHostToDevice, ctx->stream));
    ZP_HIP(ctx, hipMemcpyAsync(dbuf + o_first, buf + o_first, (total - o_first) * 8, hipMemcpyHostToDevice, ctx->stream));
    ZP_TRY(zpi_poseidon_chains(ctx, dbuf, (const unsigned char *)(dbuf + o_abs), (const unsigned int *)(dbuf + o_first), nchains, dbuf + o_out));
    ZP_HIP(ctx, hipMemcpyAsync(buf + o_out, dbuf + o_out, 160 * nsteps, hipMemcpyDeviceToHost, ctx->stream));
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t s = 0; s < nsteps; s++) memcpy(h_rates + 8 * s, buf + o_out + 20 * s + 12, 64);
    ctx->verify_counters[0] += 1;
    ctx->verify_counters[1] += nsteps;
    return ZP_OK;
}

// The commitment of every long public-input vector of a call in Goldilocks mode (csrc/verify.hip: publics_digest_host is the host's statement of the
// same): rows of 8 values, zero padded, 2^k >= 2 rows, the binary tree of zp_merkle_commit_rows, tree after tree on the stream; the roots come back in
// one copy after one synchronisation.  One buffer: [rows of every vector][tree of every vector][roots]
int32_t zpi_publics_digests(zp_ctx *ctx, const std::vector<const std::vector<u64> *> &pubs, u64 *h_out4) {
    ZP_BIND(ctx);
    const size_t n = pubs.size();
    if (!n) return ZP_OK;
    std::vector<size_t> rows(n), row_at(n), tree_at(n);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        size_t M = 2;
        while (M * 8 < pubs[i]->size()) M <<= 1;
        rows[i] = M; row_at[i] = at; at += 8 * M;
    }
    const size_t n_rows = at;
    for (size_t i = 0; i < n; i++) { tree_at[i] = at; at += 4 * (2 * rows[i] - 1); }
    const size_t o_roots = at, total = at + 4 * n;
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void *stv = nullptr;
    ZP_TRY(zpi_pinned(ctx, (n_rows > 4 * n ? n_rows : 4 * n) * 8, &stv));
    u64 *buf = (u64 *)stv, *dbuf = nullptr;
    for (size_t i = 0; i < n; i++) {
        memcpy(buf + row_at[i], pubs[i]->data(), 8 * pubs[i]->size());
        memset(buf + row_at[i] + pubs[i]->size(), 0, 8 * (8 * rows[i] - pubs[i]->size()));
    }
    ZP_TRY(zpi_scratch(ctx, 3, total, &dbuf));
    ZP_HIP(ctx, hipMemcpyAsync(dbuf, buf, n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
    for (size_t i = 0; i < n; i++) {
        ZP_TRY(commit_tree<true>(ctx, dbuf + row_at[i], rows[i], 8, dbuf + tree_at[i]));
        ZP_HIP(ctx, hipMemcpyAsync(dbuf + o_roots + 4 * i, dbuf + tree_at[i] + 4 * (2 * rows[i] - 2), 32, hipMemcpyDeviceToDevice, ctx->stream));
    }
    ZP_HIP(ctx, hipMemcpyAsync(buf, dbuf + o_roots, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(h_out4, buf, 32 * n);
    return ZP_OK;
}

// the leaf hash and the path of `count` openings in one launch (openings_walk_kernel)
int32_t zpi_poseidon_openings_walk(zp_ctx *ctx, const u64 *d_op, const u64 *d_vals, u64 mw, const u64 *d_index, const u64 *d_sib, const u64 *d_sib_off,
                                   size_t count, u64 *d_inputs, u64 *d_digests) {
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    if (!count) return ZP_OK;
    hipLaunchKernelGGL(openings_walk_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream, d_op, d_vals, mw, d_index, d_sib, d_sib_off, d_inputs, d_digests,
                       ctx->d_rc, ctx->d_mds);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

// The openings of a verifier in one call.  From `verify_lane_min` openings on: the lane-per-opening kernel (packed word-major, one upload, one
// launch, one download); below it the 12-lane walk kernel of the recursion witness, fed a scratch buffer for the permutation inputs it writes, and
// the digests compared here.  Both give the same flags (tests/test_gpu_stark_verify.py forces each through the knob).  Both are packed straight
// into the ctx's pinned staging buffer (a batch of chunk proofs is tens of MB: no pageable copy, and nothing the copy reads dies on an early return)
// and their results come back through it.  One synchronisation after the launch (the one before packing finds an idle stream: it only keeps an
// earlier small copy from still reading the staging buffer).
int32_t zpi_merkle_verify_openings(zp_ctx *ctx, const ZpOpening *ops, size_t n, const u64 *h_roots, size_t n_roots, uint8_t *ok) {
    if (!n) return ZP_OK;
    ZP_ARG(ctx, ops && h_roots && ok && n < (1u << 28) && n_roots >= 1 && n_roots < (1u << 28), "bad openings");
    for (size_t o = 0; o < n; o++)
        ZP_ARG(ctx, ops[o].values && (ops[o].path || !ops[o].depth) && ops[o].width >= 1 && ops[o].width < (1u << 16) && ops[o].depth <= 40 &&
                        ops[o].root_slot < n_roots, "opening out of range");
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    const bool lane_form = n >= (size_t)(ctx->tune_verify_lane_min > 0 ? ctx->tune_verify_lane_min : 256);      // 256: unmeasured (ctx.hpp)
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void *stv = nullptr;
    if (lane_form) {
        // segments: runs of one (width, depth) in the caller's order
        std::vector<VerifySeg> segs;
        std::vector<u32> seg_of(n);
        size_t nv = 0, ns = 0;
        for (size_t o = 0; o < n; o++) {
            if (segs.empty() || segs.back().width != ops[o].width || segs.back().depth != ops[o].depth) {
                if (!segs.empty()) { nv += (size_t)segs.back().width * segs.back().n; ns += (size_t)segs.back().depth * 4 * segs.back().n; }
                segs.push_back({(u64)nv, (u64)ns, (u32)o, 0u, ops[o].width, ops[o].depth});
            }
            segs.back().n++;
            seg_of[o] = (u32)(segs.size() - 1);
        }
        nv += (size_t)segs.back().width * segs.back().n; ns += (size_t)segs.back().depth * 4 * segs.back().n;
        // one buffer: [segments][segment of an opening (u32)][root slot (u32)][index][roots][values][siblings][flags]
        const size_t w_seg = segs.size() * (sizeof(VerifySeg) / 8), w_u32 = (n + 1) / 2, o_segof = w_seg, o_slot = o_segof + w_u32, o_idx = o_slot + w_u32,
                     o_roots = o_idx + n, o_vals = o_roots + 4 * n_roots, o_sibs = o_vals + nv, o_ok = o_sibs + ns, total = o_ok + (n + 7) / 8;
        static_assert(sizeof(VerifySeg) % 8 == 0, "segment records are whole words");
        ZP_TRY(zpi_pinned(ctx, total * 8, &stv));
        u64 *buf = (u64 *)stv;
        memcpy(buf, segs.data(), segs.size() * sizeof(VerifySeg));
        buf[o_slot - 1] = buf[o_idx - 1] = 0;              // the odd half word behind each u32 array
        memcpy(buf + o_segof, seg_of.data(), n * 4);
        u32 *slot = (u32 *)(buf + o_slot);
        for (size_t o = 0; o < n; o++) { slot[o] = ops[o].root_slot; buf[o_idx + o] = ops[o].index; }
        // the transpose to word-major in tiles of 64 openings: the writes run along the openings (one wave's worth of consecutive words per row),
        // the reads stay inside the 64 rows of the tile
        for (const VerifySeg &sg : segs)
            for (size_t i0 = 0; i0 < sg.n; i0 += 64) {
                const size_t i1 = i0 + 64 < sg.n ? i0 + 64 : sg.n;
                u64 *v = buf + o_vals + sg.voff, *sb = buf + o_sibs + sg.soff;
                for (u32 k = 0; k < sg.width; k++)
                    for (size_t i = i0; i < i1; i++) v[(size_t)k * sg.n + i] = ops[sg.o0 + i].values[k];
                for (u32 k = 0; k < 4 * sg.depth; k++)
                    for (size_t i = i0; i < i1; i++) sb[(size_t)k * sg.n + i] = ops[sg.o0 + i].path[k];
            }
        memcpy(buf + o_roots, h_roots, 32 * n_roots);
        u64 *d = nullptr;
        ZP_TRY(zpi_scratch(ctx, 3, total, &d));
        ZP_HIP(ctx, hipMemcpyAsync(d, buf, o_ok * 8, hipMemcpyHostToDevice, ctx->stream));
        launch_mds(ctx, openings_lane_kernel<true>, openings_lane_kernel<false>, (n + 255) / 256, (const VerifySeg *)d, (const u32 *)(d + o_segof), (const u32 *)(d + o_slot),
                   d + o_idx, d + o_roots, d + o_vals, d + o_sibs, n, (unsigned char *)(d + o_ok));
        ZP_HIP(ctx, hipGetLastError());
        ZP_HIP(ctx, hipMemcpyAsync(buf + o_ok, d + o_ok, n, hipMemcpyDeviceToHost, ctx->stream));
        ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(ok, buf + o_ok, n);
        return ZP_OK;
    }
    // latency form: rows of mw words per opening, the siblings one opening after the other
    u64 mw = 4, nsib = 0, nperm = 0;
    for (size_t o = 0; o < n; o++) { if (ops[o].width > mw) mw = ops[o].width; nsib += 4 * (u64)ops[o].depth; }
    const size_t o_op = 0, o_idx = 3 * n, o_off = o_idx + n, o_vals = o_off + n, o_sib = o_vals + n * mw, o_dig = o_sib + nsib, o_in_at = o_dig + 4 * n;
    ZP_TRY(zpi_pinned(ctx, o_in_at * 8, &stv));
    u64 *buf = (u64 *)stv;
    memset(buf + o_vals, 0, n * mw * 8);                   // a row shorter than its last block of 8 ends in zeros
    nsib = 0;
    for (size_t o = 0; o < n; o++) {
        const u64 na = ops[o].width > 4 ? (ops[o].width + 7) / 8 : 0;
        buf[o_op + 3 * o] = nperm; buf[o_op + 3 * o + 1] = na; buf[o_op + 3 * o + 2] = ops[o].depth;
        buf[o_idx + o] = ops[o].index;
        buf[o_off + o] = nsib;
        memcpy(&buf[o_vals + o * mw], ops[o].values, 8 * (size_t)ops[o].width);
        if (ops[o].depth) memcpy(&buf[o_sib + nsib], ops[o].path, 32 * (size_t)ops[o].depth);
        nsib += 4 * (u64)ops[o].depth;
        nperm += na + ops[o].depth;
    }
    u64 *d = nullptr;
    ZP_TRY(zpi_scratch(ctx, 3, o_in_at + 12 * nperm, &d));
    ZP_HIP(ctx, hipMemcpyAsync(d, buf, o_dig * 8, hipMemcpyHostToDevice, ctx->stream));
    ZP_TRY(zpi_poseidon_openings_walk(ctx, d + o_op, d + o_vals, mw, d + o_idx, d + o_sib, d + o_off, n, d + o_in_at, d + o_dig));
    const u64 *dig = buf + o_dig;
    ZP_HIP(ctx, hipMemcpyAsync(buf + o_dig, d + o_dig, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t o = 0; o < n; o++) ok[o] = memcmp(&dig[4 * o], h_roots + 4 * (size_t)ops[o].root_slot, 32) == 0 ? 1 : 0;
    return ZP_OK;
}

extern "C" {

int32_t zp_poseidon_perm(zp_ctx *ctx, uint64_t *d_states, size_t count) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "poseidon_perm");
    if (count == 0) return ZP_OK;
    ZP_ARG(ctx, d_states != nullptr, "null device pointer");
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    if (count <= 64) {   // latency-bound regime: spread each state over 12 lanes
        hipLaunchKernelGGL(poseidon_perm_small_kernel, dim3((unsigned)((count + 4) / 5)), dim3(64), 0, ctx->stream,
                           (u64 *)d_states, (int)count, ctx->d_rc, ctx->d_mds);
        ZP_HIP(ctx, hipGetLastError());
        return ZP_OK;
    }
    launch_mds(ctx, poseidon_perm_kernel<true>, poseidon_perm_kernel<false>, (count + 255) / 256, (u64 *)d_states, count);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

int32_t zp_poseidon_trace(zp_ctx *ctx, const uint64_t *d_inputs, size_t count, uint64_t *d_states, uint64_t *d_cubes, size_t stride) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "poseidon_trace");
    if (count == 0) return ZP_OK;
    ZP_ARG(ctx, d_inputs && d_states && d_cubes, "null device pointer");
    ZP_ARG(ctx, stride >= 32 * count, "column stride smaller than 32 rows per permutation");
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    hipLaunchKernelGGL(poseidon_trace_kernel, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, ctx->stream, (const u64 *)d_inputs, count,
                       (u64 *)d_states, (u64 *)d_cubes, stride, ctx->d_rc, ctx->d_mds);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

int32_t zp_poseidon_sponge_caps(zp_ctx *ctx, uint64_t *h_state, const uint64_t *h_blocks, size_t nblocks, size_t extra, uint64_t *h_rates,
                                uint64_t *h_caps) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "poseidon_sponge");
    ZP_ARG(ctx, h_state && h_rates && (h_blocks || nblocks == 0), "null pointer");
    ZP_ARG(ctx, nblocks <= 65536 && extra <= 65536, "too many blocks");
    for (int i = 0; i < 12; i++) ZP_ARG(ctx, h_state[i] < GL_P, "state not canonical");
    for (size_t i = 0; i < nblocks * 8; i++) ZP_ARG(ctx, h_blocks[i] < GL_P, "block not canonical");
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    // one buffer, [state][blocks] in and [state] ... [rates][caps] out (poseidon_sponge_kernel), packed and unpacked here once.  The usual case (a
    // transcript step is a few dozen blocks, 48 KiB of input at the most): the ctx's pinned staging buffer, which the kernel reads and writes itself;
    // above that a pageable copy and device scratch
    const size_t nin = 12 + nblocks * 8, nout = (1 + extra) * 8, ncap = h_caps ? ((nblocks ? nblocks : 1) + extra) * 4 : 0, total = nin + nout + ncap;
    const bool staged = nin * 8 <= 48 * 1024;
    std::vector<u64> pageable(staged ? 0 : total);
    u64 *h = pageable.data(), *d = nullptr;
    if (staged) {
        void *stv = nullptr;
        ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));       // the staging buffer may still feed an earlier small copy
        ZP_TRY(zpi_pinned(ctx, total * 8, &stv));
        h = (u64 *)stv;
    } else {
        ZP_TRY(zpi_scratch(ctx, 3, total, &d));
    }
    memcpy(h, h_state, 96);
    if (nblocks) memcpy(h + 12, h_blocks, nblocks * 64);
    if (staged) {
        hipLaunchKernelGGL(poseidon_sponge_kernel<true>, dim3(1), dim3(64), nin * 8, ctx->stream, h, (int)nblocks, (int)extra, ctx->d_rc, ctx->d_mds,
                           h_caps ? 1 : 0);
        ZP_HIP(ctx, hipGetLastError());
        ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        ZP_TRY(zpi_h2d_small(ctx, d, h, nin * 8));
        hipLaunchKernelGGL(poseidon_sponge_kernel<false>, dim3(1), dim3(64), 0, ctx->stream, d, (int)nblocks, (int)extra, ctx->d_rc, ctx->d_mds,
                           h_caps ? 1 : 0);
        ZP_HIP(ctx, hipGetLastError());
        // state and rates are not adjacent (the blocks sit between them): two small copies
        ZP_TRY(zpi_d2h_small(ctx, h, d, 96));
        ZP_TRY(zpi_d2h_small(ctx, h + nin, d + nin, (nout + ncap) * 8));
    }
    memcpy(h_state, h, 96);
    memcpy(h_rates, h + nin, nout * 8);
    if (h_caps) memcpy(h_caps, h + nin + nout, ncap * 8);
    return ZP_OK;
}

int32_t zp_poseidon_sponge(zp_ctx *ctx, uint64_t *h_state, const uint64_t *h_blocks, size_t nblocks, size_t extra, uint64_t *h_rates) {
    return zp_poseidon_sponge_caps(ctx, h_state, h_blocks, nblocks, extra, h_rates, nullptr);
}

int32_t zp_pow_grind(zp_ctx *ctx, const uint64_t *h_seed4, int32_t bits, uint64_t *h_nonce) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "pow_grind");
    ZP_ARG(ctx, h_seed4 && h_nonce, "null pointer");
    ZP_ARG(ctx, bits >= 0 && bits <= 40, "bits must be in [0,40]");
    for (int i = 0; i < 4; i++) ZP_ARG(ctx, h_seed4[i] < GL_P, "seed not canonical");
    if (bits == 0) { *h_nonce = 0; return ZP_OK; }
    ZP_TRY(zpi_poseidon_sync_tables(ctx));
    u64 *d;   // [0..3] seed, [4] best nonce of the batch
    ZP_TRY(zpi_scratch(ctx, 3, 8, &d));
    u64 h[5] = {h_seed4[0], h_seed4[1], h_seed4[2], h_seed4[3], ~0ULL};
    ZP_TRY(zpi_h2d_small(ctx, d, h, sizeof(h)));
    const u64 batch = 1ULL << (bits >= 16 ? 20 : bits + 4);   // expected hits per batch: 16 (fewer for bits >= 16)
    for (u64 base = 0;; base += batch) {
        ZP_ARG(ctx, base < (1ULL << 50), "no proof-of-work nonce below 2^50");
        launch_mds(ctx, pow_grind_kernel<true>, pow_grind_kernel<false>, batch / 256, (const u64 *)d, (int)bits, base, d + 4);
        ZP_HIP(ctx, hipGetLastError());
        u64 best;
        ZP_TRY(zpi_d2h_small(ctx, &best, d + 4, sizeof(best)));
        if (best != ~0ULL) { *h_nonce = best; return ZP_OK; }
    }
}

int32_t zp_merkle_commit(zp_ctx *ctx, const uint64_t *d_cols, size_t M, int32_t W, uint64_t *d_tree) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "merkle_commit");
    ZP_ARG(ctx, M >= 1 && (M & (M - 1)) == 0, "M must be a power of two");
    ZP_ARG(ctx, W >= 1, "W must be >= 1");
    ZP_ARG(ctx, d_cols && d_tree, "null device pointer");
    return commit_tree<false>(ctx, (const u64 *)d_cols, M, (size_t)W, (u64 *)d_tree);
}

int32_t zp_merkle_commit_rows(zp_ctx *ctx, const uint64_t *d_rows, size_t M, size_t len, uint64_t *d_tree) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "merkle_commit_rows");
    ZP_ARG(ctx, M >= 1 && (M & (M - 1)) == 0, "M must be a power of two");
    ZP_ARG(ctx, len >= 1, "len must be >= 1");
    ZP_ARG(ctx, d_rows && d_tree, "null device pointer");
    return commit_tree<true>(ctx, (const u64 *)d_rows, M, len, (u64 *)d_tree);
}

int32_t zp_merkle_open(zp_ctx *ctx, const uint64_t *d_tree, size_t M, size_t idx, uint64_t *h_path) {
    if (!ctx) return ZP_ERR_ARG;
    ZP_BIND(ctx);
    ZP_ARG(ctx, M >= 1 && (M & (M - 1)) == 0, "M must be a power of two");
    ZP_ARG(ctx, idx < M, "leaf index out of range");
    ZP_ARG(ctx, d_tree && h_path, "null pointer");
    const u64 *lvl = (const u64 *)d_tree;
    size_t cnt = M;
    int d = 0;
    while (cnt > 1) {
        ZP_HIP(ctx, hipMemcpyAsync(h_path + 4 * d, lvl + (idx ^ 1) * 4, 4 * sizeof(u64), hipMemcpyDeviceToHost,
                                   ctx->stream));
        lvl += cnt * 4;
        cnt >>= 1;
        idx >>= 1;
        d++;
    }
    ZP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZP_OK;
}

// n openings into ONE binary tree (see the header): the device primitive of the verifier on its own
int32_t zp_merkle_verify_batch(zp_ctx *ctx, const uint64_t *h_values, size_t width, const uint64_t *h_index, const uint64_t *h_paths, int32_t depth,
                               const uint64_t *h_root4, size_t n, uint8_t *h_ok) {
    if (!ctx) return ZP_ERR_ARG;
    ZpStage stage_(ctx, "merkle_verify_batch");
    try {
        if (n == 0) return ZP_OK;
        ZP_ARG(ctx, h_values && h_index && h_root4 && h_ok && (h_paths || depth == 0), "null pointer");
        ZP_ARG(ctx, width >= 1 && width < (1u << 16) && depth >= 0 && depth <= 40 && n < (1u << 28), "width, depth or count out of range");
        // field elements are read mod p, as the hash takes them; an index beyond the tree is no opening of it
        std::vector<u64> v(n * width), p((size_t)depth * 4 * n), root(h_root4, h_root4 + 4);
        for (size_t i = 0; i < v.size(); i++) v[i] = gl_canon(h_values[i]);
        for (size_t i = 0; i < p.size(); i++) p[i] = gl_canon(h_paths[i]);
        std::vector<ZpOpening> ops(n);
        for (size_t o = 0; o < n; o++) ops[o] = {&v[o * width], depth ? &p[o * (size_t)depth * 4] : nullptr, h_index[o], (uint32_t)width, (uint32_t)depth, 0u};
        ZP_TRY(zpi_merkle_verify_openings(ctx, ops.data(), n, root.data(), 1, h_ok));
        for (size_t o = 0; o < n; o++)
            if (depth < 64 && (h_index[o] >> depth)) h_ok[o] = 0;
        return ZP_OK;
    } catch (const std::bad_alloc &) {
        try { ctx->err = "out of host memory"; } catch (...) {}
        return ZP_ERR_NOMEM;
    } catch (...) {
        return ZP_ERR_INTERNAL;
    }
}

int32_t zp_merkle_commit_host(zp_ctx *ctx, const uint64_t *h_cols, size_t M, int32_t W, uint64_t *h_tree) {
    if (!ctx) return ZP_ERR_ARG;
    ZP_BIND(ctx);
    ZP_ARG(ctx, M >= 1 && (M & (M - 1)) == 0, "M must be a power of two");
    ZP_ARG(ctx, W >= 1 && h_cols && h_tree, "bad arguments");
    const size_t bin = (size_t)W * M * sizeof(u64), bt = (2 * M - 1) * 4 * sizeof(u64);
    void *dc = nullptr, *dt = nullptr;
    ZP_TRY(zp_dev_alloc(ctx, bin, &dc));
    int32_t rc = zp_dev_alloc(ctx, bt, &dt);
    if (rc == ZP_OK) rc = zp_h2d(ctx, dc, h_cols, bin);
    if (rc == ZP_OK) rc = zp_merkle_commit(ctx, (const uint64_t *)dc, M, W, (uint64_t *)dt);
    if (rc == ZP_OK) rc = zp_d2h(ctx, h_tree, dt, bt);
    (void)zp_dev_free(ctx, dc);
    (void)zp_dev_free(ctx, dt);
    return rc;
}

}  // extern "C"
