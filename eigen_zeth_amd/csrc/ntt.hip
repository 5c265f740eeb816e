// Goldilocks NTT / iNTT / LDE for gfx950.
//
// No reference counterpart exists in /root/reference (the prover arithmetic is external to
// eigen-zeth); reference call site served: src/prover/provider.rs:358-377
// (GenChunkProof).  Algorithm: Stockham auto-sort, decimation in frequency, m = ceil(logN/9)
// out-of-place passes of radix R = 2^L (L = 6..9).  Pass i views the column as [R][N/R], a
// workgroup owns a tile of T = 32 consecutive u in [0, N/R):
//     a_r = in[r*(N/R) + u]                               (R segments of T*8 = 256 contiguous bytes)
//     b_k = (sum_r a_r w_R^(rk)) * w_N^(Pprev*k*s)          u = s*Pprev + c,  Pprev = R_1*...*R_(i-1)
//     out[s*Pprev*R + k*Pprev + c] = b_k                    (segments of >= 256 contiguous bytes)
// so natural order goes in and natural order comes out with every global access coalesced in
// 256-byte runs and no separate transpose / bit-reversal pass.  Inside a tile the R-point DFT is
// 2-3 rounds of register radix-2^A (A <= 4, 16 elements per thread, shift-only butterflies) exchanged
// through LDS with an XOR swizzle so that both the row accesses and the transposing copy-out of pass 1 are
// bank-conflict free (MI355X_MICROARCH.md, LDS: ds_read_b64 = 2x32 lanes over 64 banks).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ctx.hpp"
#include "wave_xchg.hpp"
#include "gl_asm.hpp"
#include "gl_limb.hpp"
#include "ntt_geo.hpp"

// the data of a pass is touched exactly once: non-temporal loads/stores (measured +1 % on the 2^24 bench, same results)
#define ZP_LDG(p) __builtin_nontemporal_load(p)
#define ZP_STG(p, v) __builtin_nontemporal_store(v, p)

namespace {

typedef __attribute__((ext_vector_type(4))) int zp_i32x4;
typedef __attribute__((address_space(1))) u64 zp_gu64;     // global memory, said so: an address that went through sgpr_opaque has lost what the compiler inferred
typedef __attribute__((address_space(1))) char zp_gchar;
typedef __attribute__((address_space(3))) u64 zp_lu64;

// A word of the tile by its LDS byte address.  ntt_pass2_kernel and lde_seam_kernel declare no static LDS, so their dynamic segment -- `lds`, the
// tile first -- starts at LDS address 0 (group_segment_fixed_size 0; the compiler itself adds that 0 to every `lds[i]`, after the point where it
// could fold it).  The factored slot addresses of ntt_geo.hpp are XORs of bit fields: they ARE the LDS address only with the base in no term,
// so these two take the address whole, and a write costs the one instruction that makes it.  (A static __shared__ in either kernel would
// move the segment: every NTT test fails at once.)
__device__ __forceinline__ void tile_store_at(int byte_pos, u64 x) { *(zp_lu64 *)(__UINTPTR_TYPE__)(u32)byte_pos = x; }
__device__ __forceinline__ u64 tile_load_at(int byte_pos) { return *(const zp_lu64 *)(__UINTPTR_TYPE__)(u32)byte_pos; }

// A wave-uniform value the compiler may not look through: what is computed from it is computed where it is used (in scalar registers), not
// ahead of the loop and kept.  No instruction.
template <bool ON>
__device__ __forceinline__ u64 sgpr_opaque(u64 x) {
    if constexpr (!ON) return x;
    u32 lo = (u32)x, hi = (u32)(x >> 32);   // (as two halves: a 64-bit scalar operand does not get through instruction selection)
    asm("" : "+s"(lo), "+s"(hi));
    return ((u64)hi << 32) | lo;
}
template <bool ON>
__device__ __forceinline__ int sgpr_opaque_once(int x) {   // of a loop-invariant value: once per evaluation, not once per kernel
    if constexpr (!ON) return x;
    asm volatile("" : "+s"(x));
    return x;
}

// the per-tile table of a pass of ntt_pass2_kernel, fixed by the plan for every launch
constexpr int TAB_NONE = 0, TAB_FIXED = 1 /* output side, the same for every tile */, TAB_TILE = 2 /* output side, per tile */, TAB_IN = 3 /* input side */;

struct PassArgs {
    const u64 *in;
    u64 *out;
    u64 in_cs, out_cs;  // column strides in elements
    u64 in_valid;       // elements per input column that are real; the rest reads as zero
    const u64 *twl, *twh;
    const u64 *tws;
    const u64 *tw1;        // transposing pass, table form: w^(u k) at [u * R + k] (MODE 3)
    const u64 *itab;       // last pass, input side: the inter-pass twiddle the pass before it left out (times 1/N of an inverse plan) at [k * R + row]; null: none
    const u64 *csl, *csh;  // coset post-scale tables (last pass of the inverse transform in LDE)
    u64 scale;
    int logn, logPprev, lb, cslb;
    int j0inv;  // w_16(user) = (2^12)^j0, j0inv = j0^-1 mod 16; 0 = root not a power of two path (generic twiddles)
    int logPin;  // itab: k = u0 >> logPin, the Pprev of the pass before this one
    int flags;  // 1: inter-pass twiddle  2: multiply by `scale`  4: coset post-scale  8: a middle pass (MODE 1 whether it multiplies or not)
    int ncols;  // MODE 3: the grid is one-dimensional, columns of one launch
};

__device__ __forceinline__ u64 tw_lookup(const u64 *lo, const u64 *hi, int lb, u64 e) {
    u64 a = lo[e & ((1ULL << lb) - 1)];
    u64 b = hi[e >> lb];
    return gl_mul(a, b);
}

// radix-2^A DIF with the canonical root c = 2^12 (order 16): every twiddle is a shift.
// v[p] receives DFT_c[brev(p)];  the caller maps that to the user's root, w_16 = c^j0:
// DFT_user[k'] = DFT_c[j0*k' mod 2^A]  =>  register p holds user index  k' = j0inv*brev(p) mod 2^A.
__device__ __forceinline__ u64 mul_c16(int e, u64 d) {   // e is a constant after unrolling: the switch folds away
    switch (e) {                                          // x * 2^(12 e): hand-written forms of gl_asm.hpp
        case 0: return d;
        case 1: return gl_shl12<1>(d);
        case 2: return gl_shl12<2>(d);
        case 3: return gl_shl12<3>(d);
        case 4: return gl_shl12<4>(d);
        case 5: return gl_shl12<5>(d);
        case 6: return gl_shl12<6>(d);
        default: return gl_shl12<7>(d);
    }
}
// butterflies two at a time through the hand-scheduled carry chains of gl_asm.hpp (x+y, x-y canonical)
template <int A>
__device__ __forceinline__ void dif_shift(u64 *v) {
    static_assert(A >= 2 && A <= 4, "radix 4, 8 or 16");
#pragma unroll
    for (int s = 0; s < A; s++) {
        const int half = 1 << (A - 1 - s);
#pragma unroll
        for (int t = 0; t < (1 << (A - 1)); t += 2) {
            const int i0 = (t / half) * 2 * half + (t % half), i1 = ((t + 1) / half) * 2 * half + ((t + 1) % half);
            gl_bfly2(v[i0], v[i0 + half], v[i1], v[i1 + half]);
            v[i0 + half] = mul_c16((t % half) * (8 / half), v[i0 + half]);
            v[i1 + half] = mul_c16(((t + 1) % half) * (8 / half), v[i1 + half]);
        }
    }
}

// Workgroup barrier that orders LDS traffic only: unlike __syncthreads() it does not drain vmcnt, so
// the next tile's global loads (and the previous tile's stores) stay in flight across it.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the read half of an exchange: the inputs of the next round (radix 2^ANEXT at bit POSNEXT of the slot) from LDS
template <typename G, int ANEXT, int POSNEXT>
__device__ __forceinline__ void exchange_read(u64 *v, const u64 *lds, int tid) {
    constexpr int GN = 16 >> ANEXT;
#pragma unroll
    for (int g = 0; g < GN; g++) {
        const int gamma = g * G::NT + tid;
        const int t = gamma & (G::T - 1), o = gamma >> G::LT;
#pragma unroll
        for (int j = 0; j < (1 << ANEXT); j++)
            v[g * (1 << ANEXT) + j] = lds[G::lpos(slot_of(o, j, POSNEXT, ANEXT), t)];
    }
}

// twr: LDS copy of w_(2^(POS+A))^e (TWSH = 0) or, for the radix-2^11 / 2^12 passes whose LDS is all tile, the global
// table of w_4096^e (TWSH = 12 - (POS + A)); 32 KiB, read by every workgroup, L2 / L1 resident
template <typename G, int A, int POS, int ANEXT, int POSNEXT, int TWSH, bool FACT = true>
__device__ __forceinline__ void exchange2(u64 *v, u64 *lds, const u64 *twr, int j0inv, int tid) {
    constexpr int GR = 16 >> A;
#pragma unroll
    for (int g = 0; g < GR; g++) {
        const int gamma = g * G::NT + tid;
        const int t = gamma & (G::T - 1), o = gamma >> G::LT;
        const int rho = o & ((1 << POS) - 1);
        // w_(2^(POS+A))^(kj*rho) from the LDS copy; p = 0 needs none, the rest go two products at a time
        {
            const int kj1 = (j0inv * brev(1, A)) & ((1 << A) - 1);
            v[g * (1 << A) + 1] = gl_mul1(v[g * (1 << A) + 1], twr[(kj1 * rho) << TWSH]);
        }
#pragma unroll
        for (int p = 2; p < (1 << A); p += 2) {
            const int kja = (j0inv * brev(p, A)) & ((1 << A) - 1), kjb = (j0inv * brev(p + 1, A)) & ((1 << A) - 1);
            gl_mul2(v[g * (1 << A) + p], twr[(kja * rho) << TWSH], v[g * (1 << A) + p + 1], twr[(kjb * rho) << TWSH]);
        }
        // The slot of register p takes the runtime k_j twice: as the round's field and, where that field reaches k's low bits, in the column
        // swizzle.  Factored (ntt_geo.hpp): the lane's part once per round, the two uniform parts of k_j in scalar registers, one XOR per
        // write.  Written out as lpos(slot_of(o, kj, ..), t) the compiler rebuilt the whole position for every register: five VALU a write.
        // The tiles of 8 columns and fewer with three rounds (slot swizzle: radix 2^11, 2^12) keep lpos, and so does a first pass on the
        // per-lane twiddle chain (FACT false): it spills already, and the lane part held across a round's writes costs it more scratch.
        if constexpr (G::FACTORED && FACT) {
            const int lane = G::wr_lane(o, t, POS, A);
#pragma unroll
            for (int p = 0; p < (1 << A); p++) {
                const int kj = (j0inv * brev(p, A)) & ((1 << A) - 1);  // wave-uniform
                tile_store_at(lane ^ G::wr_uni(kj, POS, A), v[g * (1 << A) + p]);
            }
        } else {
#pragma unroll
            for (int p = 0; p < (1 << A); p++) {
                const int kj = (j0inv * brev(p, A)) & ((1 << A) - 1);  // wave-uniform
                lds[G::lpos(slot_of(o, kj, POS, A), t)] = v[g * (1 << A) + p];
            }
        }
    }
    lds_barrier();
    exchange_read<G, ANEXT, POSNEXT>(v, lds, tid);
}

// ---- the same two building blocks on four signed 24-bit-position limbs (gl_limb.hpp): butterflies are carry-free 32-bit adds, every
// twiddle 2^(24 j) a renaming of limbs, and the canonical 64-bit value comes back inside the twiddle product that follows a round
template <int E>
__device__ __forceinline__ gl_l4 mul_c16_l4(const gl_l4 &d) { return gl_l4_mul_c16<E>(d); }
__device__ __forceinline__ gl_l4 mul_c16_l4(int e, const gl_l4 &d) {   // e is a constant after unrolling
    switch (e) {
        case 0: return d;
        case 1: return gl_l4_mul_c16<1>(d);
        case 2: return gl_l4_mul_c16<2>(d);
        case 3: return gl_l4_mul_c16<3>(d);
        case 4: return gl_l4_mul_c16<4>(d);
        case 5: return gl_l4_mul_c16<5>(d);
        case 6: return gl_l4_mul_c16<6>(d);
        default: return gl_l4_mul_c16<7>(d);
    }
}
// the A butterfly levels on limb-form values: x[p] <- DFT_c[brev(p)], limbs grow by one bit per level
template <int A>
__device__ __forceinline__ void dif_levels_l4(gl_l4 *x) {
    static_assert(A >= 2 && A <= 4, "radix 4, 8 or 16");
#pragma unroll
    for (int s = 0; s < A; s++) {
        const int half = 1 << (A - 1 - s);
#pragma unroll
        for (int t = 0; t < (1 << (A - 1)); t++) {
            const int i0 = (t / half) * 2 * half + (t % half);
            const gl_l4 a = x[i0], b = x[i0 + half];
            x[i0] = gl_l4_add(a, b);
            x[i0 + half] = mul_c16_l4((t % half) * (8 / half), gl_l4_sub(a, b));
        }
    }
}
// x[p] receives DFT_c[brev(p)] of the canonical values v[0 .. 2^A), |limbs| < 2^(24 + A)
template <int A>
__device__ __forceinline__ void dif_shift_l4(const u64 *v, gl_l4 *x) {
#pragma unroll
    for (int i = 0; i < (1 << A); i++) x[i] = gl_l4_from(v[i]);
    dif_levels_l4<A>(x);
}
// the LDS record of a factor: balanced words of w B^i, i < 4 (32 bytes)
__device__ __forceinline__ gl_w4 w4_load(const gl_w4 *p) {
    const zp_i32x4 a = *(const zp_i32x4 *)p->lo, b = *(const zp_i32x4 *)p->hi;
    gl_w4 w;
    w.lo[0] = a.x; w.lo[1] = a.y; w.lo[2] = a.z; w.lo[3] = a.w;
    w.hi[0] = b.x; w.hi[1] = b.y; w.hi[2] = b.z; w.hi[3] = b.w;
    return w;
}
__device__ __forceinline__ void w4_store(gl_w4 *p, const u64 w0, const u64 w1, const u64 w2, const u64 w3) {
    i32 l[4], h[4];
    gl_l4_balance(w0, l[0], h[0]);
    gl_l4_balance(w1, l[1], h[1]);
    gl_l4_balance(w2, l[2], h[2]);
    gl_l4_balance(w3, l[3], h[3]);
    zp_i32x4 a = {l[0], l[1], l[2], l[3]}, b = {h[0], h[1], h[2], h[3]};
    *(zp_i32x4 *)p->lo = a;
    *(zp_i32x4 *)p->hi = b;
}
// twr4: LDS records of w_(2^(POS+A))^e
template <typename G, int A, int POS, int ANEXT, int POSNEXT>
__device__ __forceinline__ void exchange2_l4(const gl_l4 *x, u64 *v, u64 *lds, const gl_w4 *twr4, int j0inv, int tid) {
    constexpr int GR = 16 >> A;
#pragma unroll
    for (int g = 0; g < GR; g++) {
        const int gamma = g * G::NT + tid;
        const int t = gamma & (G::T - 1), o = gamma >> G::LT;
        const int rho = o & ((1 << POS) - 1);
#pragma unroll
        for (int p = 0; p < (1 << A); p++) {
            const int kj = (j0inv * brev(p, A)) & ((1 << A) - 1);  // wave-uniform
            const u64 y = p == 0 ? gl_l4_canon(x[g * (1 << A)]) : gl_l4_mul(x[g * (1 << A) + p], w4_load(twr4 + kj * rho));
            lds[G::lpos(slot_of(o, kj, POS, A), t)] = y;
        }
    }
    lds_barrier();
    exchange_read<G, ANEXT, POSNEXT>(v, lds, tid);
}

// ---- the step of a tile that ntt_pass2_kernel and lde_seam_kernel share
// Table copy-out of a first pass: the tile sits in LDS, so v is dead and its registers take the 16 factors (twb: the plan's table at this tile) of the elements this lane copies out to blk
// Element i NT + tid of the tile in output order, i < 16: table entry, LDS word and destination.  Table and destination are the uniform base
// of row i, walked by scalar adds (WALK: through sgpr_opaque, as fetch_tile does), beside the lane's 32-bit byte offset 8 tid -- the table
// form is never BIG, and this offset is below 16 KiB whatever the transform.  The LDS word is the lane's rd_lane XOR a constant (ntt_geo.hpp):
// idx mod R does not depend on i, which the compiler cannot see through the opaque lane id.
template <typename G, bool WALK>
__device__ __forceinline__ void table_copy_out(u64 *v, const u64 *twb, u64 *blk, int tid) {
    constexpr int NT = G::NT;
    static_assert(G::FACTORED && NT >= G::R, "table first passes: two rounds, tiles of 16 columns or more");
    const u32 lane_bytes = (u32)tid << 3;
    u64 tw_at = sgpr_opaque<WALK>((u64)twb);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const zp_gu64 *rowp = (const zp_gu64 *)tw_at;
        tw_at = sgpr_opaque<WALK>(tw_at + 8ULL * NT);
        v[i] = *(const zp_gu64 *)((const zp_gchar *)rowp + lane_bytes);       // cacheable: the other columns of this tile hit in L2
    }
    lds_barrier();
    const int rd = G::rd_lane(tid);
    u64 st_at = sgpr_opaque<WALK>((u64)blk);
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        u64 xa = tile_load_at(rd ^ G::rd_xor(i));
        u64 xb = tile_load_at(rd ^ G::rd_xor(i + 1));
        gl_mul2(xa, v[i], xb, v[i + 1]);
        zp_gu64 *const ra = (zp_gu64 *)st_at;
        st_at = sgpr_opaque<WALK>(st_at + 8ULL * NT);
        zp_gu64 *const rb = (zp_gu64 *)st_at;
        st_at = sgpr_opaque<WALK>(st_at + 8ULL * NT);
        ZP_STG((zp_gu64 *)((zp_gchar *)ra + lane_bytes), xa);
        ZP_STG((zp_gu64 *)((zp_gchar *)rb + lane_bytes), xb);
    }
}

// Pass kernel, second generation.
//  * A workgroup walks `tiles_per_wg` consecutive tiles of one column.  ALL vector global loads of
//    tile i+1 (16 data elements per lane + the few twiddle-table entries it needs) are issued at the
//    top of iteration i and consumed in iteration i+1; the body of an iteration touches only
//    registers and LDS, and barriers order LDS only.  vmcnt is an in-order counter, so this is what
//    keeps HBM loads (and the previous tile's stores) in flight under the integer work.
//  * The loop holds two tiles a trip: the register set that receives the prefetch in one body is the current tile of the other, so no
//    register is copied from tile to tile (tiles_per_wg odd, 1 included, leaves after the first body).  Which table a pass has (TAB) is a
//    template argument, so a loop holds its own case only; uniform row and k-step addresses are walked by scalar adds where they are used
//    (sgpr_opaque) and every load and store takes a scalar base beside a 32-bit lane offset.  Before, sixteen load bases, sixteen store
//    bases and the k_j of every round were loop invariants that did not fit beside the butterflies' carry pairs and came back through
//    v_readlane.  Static counts and counters: profiles/r12_ntt_isa_breakdown.txt, r12_pmc_sq_ntt.json.  (LEAN below: the limb form and
//    the per-lane twiddle chain keep one tile a trip with a hand-over -- two bodies cost them spills.)
//  * butterflies use the canonical 16-th root 2^12 (shifts only); the user's root enters through
//    j0inv as a renaming of outputs.
//  * TRANSPOSE=false (passes 2..m, Pprev >= T): the tile shares s; the inter-pass twiddle w^(e0*k)
//    (times 1/N and the k-part of a coset power on a last pass) is a per-tile table of R entries in
//    LDS -> one multiplication per element.
//  * TRANSPOSE=true (pass 1, Pprev = 1): s = u varies with the lane; w^(u*k) is a per-lane geometric
//    chain walked in the order the shift butterflies deliver outputs: k_j = jr*i mod 2^A, so
//    h^(k_j) = (h^jr)^i * (h^-(2^A))^floor(jr*i/2^A).
//    Table form (MODE 3): the N factors w^(u*k) of a transform are the same for every column, so they are precomputed once per
//    plan in the order of the transposing copy-out ([u][k]: 8 bytes per element, coalesced) and multiplied in while the tile
//    leaves LDS -- one product per element instead of the chain's two and none of its exponent arithmetic.  What makes the
//    extra 8 bytes per element affordable is that they are read from HBM once per 8 columns: the grid is one-dimensional and
//    ordered so that the columns of one tile run next to each other on ONE XCD (workgroup id % 8 picks the XCD), and the
//    table loads are cacheable, so 7 of 8 reads are hits in that XCD's L2.
// MODE (non-transposing passes): 0 = last pass without an output product, 1 = a middle pass, or a last pass that multiplies by 1/N:
// the per-tile table on the output side where TAB says so (TAB_TILE: the inter-pass twiddle, flags & 1; TAB_FIXED: 1/N, flags & 2; TAB_NONE:
// a plain middle pass), 2 = table (TAB_FIXED) and the per-lane part of a coset power (last pass of the inverse transform in an LDE).
//    Input-side table (a.itab, MODE 0, TAB_IN): the factor w^(Pprev k s) of the pass BEFORE a last pass lands, in the last pass, on row
//    r' = s of the tile whose columns u' = k Pprev + c share k (T <= Pprev) -- again R' entries per tile and one product per element, now
//    applied to the loaded rows.  The pass before the last is then plain (integer work moves from a pass that is bound by instruction
//    issue to the one that is not), and 1/N of an inverse plan rides in the same entries: no output product at all.  The entries come
//    ready-made from the plan (itab_fill_kernel): one load per lane, a tile ahead.
// LIMB: the register butterflies and the twiddle products that follow them on the limb form of gl_limb.hpp (16 values x 4 limbs live
// between the rounds: 3 waves per SIMD, 168 VGPRs); the per-tile table and the LDS copies of the inter-round twiddles hold 32-byte
// records (the balanced words of w, w 2^24, w 2^48, w 2^72).  Not for the per-lane twiddle chain of a first pass without its table.
template <int A1, int A2, int A3, int LOGT, bool TRANSPOSE, bool PADDED, int MODE, int TAB, bool BIG = false, bool LIMB = false>
__global__ void __launch_bounds__((1 << (A1 + A2 + A3 + LOGT)) / 16, LIMB ? 3 : 4)   // 4 waves per SIMD: 128 VGPRs, of which v116..v127 are the scratch window of gl_asm.hpp
ntt_pass2_kernel(PassArgs a, int tiles_per_wg) {
    using G = Geo<A1, A2, A3, LOGT>;
    constexpr int L = G::L, R = G::R, T = G::T, NT = G::NT, AJ = G::AJ;
    constexpr int GRJ = 16 >> AJ;
    constexpr int R2 = 1 << (A2 + A3);
    constexpr bool HAS_TAB = !TRANSPOSE && MODE >= 1;
    constexpr bool TWR_LDS = L <= 10;          // radix 2^11 / 2^12: the 128 KiB tile leaves no room, twiddles come from L2
    constexpr int TPL = (R + NT - 1) / NT;     // per-tile table entries a lane prepares
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    constexpr int REC = LIMB ? 4 : 1;          // u64 per table entry (LIMB: a 32-byte gl_w4 record)
    u64 *tab = lds + R * T;                    // R entries: per-tile inter-pass twiddles (HAS_TAB)
    u64 *twr1 = tab + (HAS_TAB ? R * REC : 0); // R entries:  w_R^e      (inter-round twiddles, first exchange)
    u64 *twr2 = twr1 + R * REC;                // R2 entries: w_(R2)^e   (second exchange, 3-round passes)
    constexpr bool TW1 = TRANSPOSE && MODE == 3;
    constexpr bool CAN_IN = !TRANSPOSE && MODE == 0 && L <= 9;   // instantiations that can take the input-side table
    u64 *itl = twr2 + (TWR_LDS ? R2 * REC : 0);                  // R entries: this tile's input-side factors (a.itab)
    // The two-tile loop and the scalar address walks (below) are for the forms that gain registers by them.  The limb form's 168 registers
    // and the per-lane twiddle chain of a first pass without its table have no room for two bodies with swapped roles: they spill.
    constexpr bool LEAN = !LIMB && !(TRANSPOSE && MODE == 1);
    constexpr bool in_tab = TAB == TAB_IN;
    constexpr bool out_tab = TAB == TAB_FIXED || TAB == TAB_TILE;   // MODE 1 with TAB_NONE: a plain middle pass
    constexpr bool tile_tab = TAB == TAB_TILE;
    static_assert((!in_tab || CAN_IN) && (!out_tab || (HAS_TAB && (MODE == 1 || !tile_tab))) && (MODE != 2 || out_tab), "a table the pass has no place for");
    static_assert(!LIMB || (TWR_LDS && (TW1 || !TRANSPOSE)), "limb form: LDS twiddle copies, no per-lane twiddle chain");
    // MODE 3: one-dimensional grid; workgroup id -> (XCD x = id % 8, j = id / 8): column = j % ncols, tile group = (j / ncols) * 8 + x
    u64 col = blockIdx.y, wg_lin = blockIdx.x;
    if constexpr (TW1) {
        const u64 x = blockIdx.x & 7u, j = blockIdx.x >> 3;
        col = j % (u64)a.ncols;
        wg_lin = (j / (u64)a.ncols) * 8 + x;
    }
    const int logNR = a.logn - L;
    const int logP = a.logPprev;
    const u64 N = 1ULL << a.logn;
    const u64 *src = a.in + col * a.in_cs;
    u64 *dst = a.out + col * a.out_cs;
    u64 v[16], vn[16];
    // twiddle-table entries fetched one tile ahead (raw lo/hi halves)
    constexpr int NTW = TW1 ? 1 : TRANSPOSE ? (GRJ + 2) : (MODE == 2 ? TPL + 1 : TPL);
    u64 twl_c[NTW], twh_c[NTW], twl_n[NTW], twh_n[NTW];

    // Addressing: row j of a lane's 16 loads is  (uniform: column base + (j << POS1) rows + u0)  +  (lane: slot0 rows + t).
    // With the lane part as a 32-bit BYTE offset the loads take the scalar-base form (global_load v, voff, s[base]) and the
    // 64-bit address arithmetic -- three VALU instructions per load when written naively -- is scalar work.  The byte
    // offset fits 32 bits up to 2^28 rows; larger transforms are the BIG instantiation with 64-bit lane offsets.
    constexpr bool small_n = !BIG;
    // The uniform part walks from row to row by one scalar add (sgpr_opaque keeps it a chain: sixteen bases computed ahead and held
    // across the butterflies' carry pairs do not fit the SGPR file and end up in VGPR lanes).
    auto fetch_tile = [&](u64 *r, u64 *tl, u64 *th, u64 u0, int tid) __attribute__((always_inline)) {
        constexpr int GR = 16 >> A1;
        const u64 valid_rows = a.in_valid >> logNR;     // PADDED: rows >= valid_rows read as zero (in_valid is a multiple of N/R)
#pragma unroll
        for (int g = 0; g < GR; g++) {
            const int gamma = g * NT + tid;
            const int t = gamma & (T - 1), o = gamma >> LOGT;
            const u32 slot0 = (u32)slot_of(o, 0, G::POS1, A1);
            const u32 lane_bytes = (((u32)slot0 << logNR) + (u32)t) << 3;
            const u64 lane_el = ((u64)slot0 << logNR) + (u64)t;
            u64 row_at = sgpr_opaque<LEAN>((u64)(src + u0));                             // wave-uniform: row j starts at src + (j << POS1 rows) + u0
#pragma unroll
            for (int j = 0; j < (1 << A1); j++) {
                const zp_gu64 *rowp = (const zp_gu64 *)row_at;
                row_at = sgpr_opaque<LEAN>(row_at + ((8ULL << G::POS1) << logNR));
                const zp_gu64 *ptr;
                if constexpr (small_n) ptr = (const zp_gu64 *)((const zp_gchar *)rowp + lane_bytes);
                else ptr = rowp + lane_el;
                // short runs (T < 16) want the L2 to merge neighbouring tiles' pieces of a line: plain, cacheable loads
                u64 val;
                if constexpr (PADDED) val = (u64)(slot0 + ((u32)j << G::POS1)) < valid_rows ? (LOGT < 4 ? *ptr : ZP_LDG(ptr)) : 0ULL;
                else val = LOGT < 4 ? *ptr : ZP_LDG(ptr);
                r[g * (1 << A1) + j] = val;
            }
        }
        const u64 lm = (1ULL << a.lb) - 1;
        if constexpr (TW1) {
            (void)tl; (void)th; (void)lm;
        } else if constexpr (TRANSPOSE) {
            const int t = tid & (T - 1);
            const u64 u = u0 + t;
            const int jr = a.j0inv & ((1 << AJ) - 1);
            u64 e[NTW];
#pragma unroll
            for (int g = 0; g < GRJ; g++) e[g] = u * (u64)G::kof(((g * NT + tid) >> LOGT) << AJ);   // w^(u*klow_g)
            e[GRJ] = ((u << (L - AJ)) * (u64)jr) & (N - 1);                                       // h^jr
            e[GRJ + 1] = (N - ((u << L) & (N - 1))) & (N - 1);                                    // h^-(2^AJ) = w^-(u*R)
#pragma unroll
            for (int i = 0; i < NTW; i++) { tl[i] = a.twl[e[i] & lm]; th[i] = a.twh[e[i] >> a.lb]; }
        } else {
            if constexpr (MODE == 1) {
                if constexpr (tile_tab) {
                    const u64 e0 = (u0 >> logP) << logP;
#pragma unroll
                    for (int j = 0; j < TPL; j++) {
                        const u64 e = e0 * (u64)((tid + j * NT) & (R - 1));  // entry k = tid + j*NT (k < R used)
                        tl[j] = a.twl[e & lm];
                        th[j] = a.twh[e >> a.lb];
                    }
                }
            }
            if constexpr (CAN_IN) {
                if constexpr (in_tab) {
                    const u64 *row = a.itab + ((u0 >> a.logPin) << L);
#pragma unroll
                    for (int j = 0; j < TPL; j++) tl[j] = row[(tid + j * NT) & (R - 1)];
                }
            }
            if constexpr (MODE == 2) {
                const u64 c = (u0 + (tid & (T - 1))) & ((1ULL << logP) - 1);
                tl[TPL] = a.csl[c & ((1ULL << a.cslb) - 1)];
                th[TPL] = a.csh[c >> a.cslb];
            }
        }
    };

    // Runs shorter than a 128-byte line (T < 16) are shared between neighbouring tiles: hand neighbours to workgroups
    // of the same XCD (blockIdx % 8 -- a speed hint only, MI355X_MICROARCH.md "Workgroup dispatch") so that the other
    // parts of a line are L2 hits; measured on the bare access pattern: 2.7 -> 4.8 TB/s (profiles/r2_ubench_mem.txt)
    u64 wg = wg_lin;
    if constexpr (LOGT < 4 && !TW1) {
        if ((gridDim.x & 7u) == 0) wg = (u64)(blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    }
    const u64 tile0 = wg * tiles_per_wg;
    fetch_tile(v, twl_c, twh_c, tile0 << LOGT, threadIdx.x);
    // once per workgroup: inter-round twiddles into LDS; an output-side table that is the same for every tile (1/N, the k-part of a
    // coset power: a last pass, flags & 1 clear) is written here and stays
    {
        const int tid0 = threadIdx.x;
        if constexpr (LIMB) {
            // w 2^(24 i) = w_R^(e + i rot): 2^12 = w_16^(j0inv), so 2^24 = w_R^(j0inv R / 8) -- four entries of the same table
            for (int e = tid0; e < R; e += NT) {
                const int rot = (a.j0inv * (R / 8)) & (R - 1);
                w4_store((gl_w4 *)twr1 + e, a.tws[e << (12 - L)], a.tws[((e + rot) & (R - 1)) << (12 - L)],
                         a.tws[((e + 2 * rot) & (R - 1)) << (12 - L)], a.tws[((e + 3 * rot) & (R - 1)) << (12 - L)]);
            }
            if constexpr (G::J >= 3) {
                constexpr int L2 = A2 + A3;
                for (int e = tid0; e < R2; e += NT) {
                    const int rot = (a.j0inv * (R2 / 8)) & (R2 - 1);
                    w4_store((gl_w4 *)twr2 + e, a.tws[e << (12 - L2)], a.tws[((e + rot) & (R2 - 1)) << (12 - L2)],
                             a.tws[((e + 2 * rot) & (R2 - 1)) << (12 - L2)], a.tws[((e + 3 * rot) & (R2 - 1)) << (12 - L2)]);
                }
            }
        } else if constexpr (TWR_LDS) {
            if (tid0 < R) twr1[tid0] = a.tws[tid0 << (12 - L)];
            if constexpr (G::J >= 3) {
                if (tid0 < R2) twr2[tid0] = a.tws[tid0 << (12 - (A2 + A3))];
            }
        }
        if constexpr (HAS_TAB) {
            if constexpr (TAB == TAB_FIXED) {
#pragma unroll
                for (int j = 0; j < TPL; j++)
                    if (tid0 + j * NT < R) {
                        u64 w = (a.flags & 2) ? a.scale : 1;
                        if constexpr (MODE == 2) {
                            const u64 ek = (u64)(tid0 + j * NT) << logP;
                            const u64 ck = gl_mul(a.csl[ek & ((1ULL << a.cslb) - 1)], a.csh[ek >> a.cslb]);
                            w = (a.flags & 2) ? gl_mul(w, ck) : ck;
                        }
                        if constexpr (LIMB) w4_store((gl_w4 *)tab + tid0 + j * NT, w, gl_shl12<2>(w), gl_shl12<4>(w), gl_shl12<6>(w));
                        else tab[tid0 + j * NT] = w;
                    }
            }
        }
        if constexpr (CAN_IN) {
            if constexpr (in_tab) {
#pragma unroll
                for (int j = 0; j < TPL; j++)
                    if (tid0 + j * NT < R) itl[tid0 + j * NT] = twl_c[j];
            }
        }
    }
    lds_barrier();  // twr1/twr2 (and the first tile's itl) are read by other lanes before the first exchange barrier
    // drain the prologue loads here so that the loop is entered with nothing pending: the waitcnt
    // insertion then needs no vmcnt wait inside the body (one there would also drain the prefetch)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
    // One tile: v, twl_c, twh_c hold tile `it`, the next tile's loads go to vn, twl_n, twh_n.  The loop below calls it twice per trip with the
    // two register sets in swapped roles, so nothing is copied from tile to tile.
    auto tile_step = [&](u64 *v, u64 *twl_c, u64 *twh_c, u64 *vn, u64 *twl_n, u64 *twh_n, int it) __attribute__((always_inline)) {
        const u64 u0 = (tile0 + it) << LOGT;
        const bool more = it + 1 < tiles_per_wg;
        // opaque copy of the lane id: keeps the compiler from hoisting every per-lane address of the
        // loop body out of the loop (that costs > 100 VGPRs and spills)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        // ... and of what the uniform addresses and output renamings are made from: sixteen store bases, the k_j of every round and their
        // LDS slots are a few scalar instructions each where they are used; made ahead of the loop they outnumber the SGPRs that the
        // butterflies' carry pairs leave, and come back through v_readlane
        const int j0inv = sgpr_opaque_once<LEAN>(a.j0inv);
        const int logP = sgpr_opaque_once<LEAN>(a.logPprev);
        if (more) fetch_tile(vn, twl_n, twh_n, u0 + T, tid);

        const u64 s = TRANSPOSE ? 0 : (u0 >> logP);
        if constexpr (HAS_TAB) {
            if constexpr (tile_tab) {
#pragma unroll
                for (int j = 0; j < TPL; j++)
                    if (tid + j * NT < R) {
                        const u64 w = gl_mul(twl_c[j], twh_c[j]);
                        if constexpr (LIMB) w4_store((gl_w4 *)tab + tid + j * NT, w, gl_shl12<2>(w), gl_shl12<4>(w), gl_shl12<6>(w));
                        else tab[tid + j * NT] = w;
                    }
            }
        }
        if constexpr (CAN_IN) {
            // the rows as loaded times this tile's input-side factors (written to itl before the last barrier)
            if constexpr (in_tab) {
#pragma unroll
                for (int g = 0; g < (16 >> A1); g++) {
                    const int slot0 = slot_of((g * NT + tid) >> LOGT, 0, G::POS1, A1);
#pragma unroll
                    for (int j = 0; j < (1 << A1); j += 2)
                        gl_mul2(v[g * (1 << A1) + j], itl[(j << G::POS1) + slot0], v[g * (1 << A1) + j + 1], itl[((j + 1) << G::POS1) + slot0]);
                }
            }
        }
        gl_l4 x[LIMB ? 16 : 1];                // LIMB: the outputs of a round (the last one: x, else v)
        if constexpr (LIMB) {
#pragma unroll
            for (int g = 0; g < (16 >> A1); g++) dif_shift_l4<A1>(v + g * (1 << A1), x + g * (1 << A1));
            exchange2_l4<G, A1, G::POS1, A2, G::POS2>(x, v, lds, (const gl_w4 *)twr1, j0inv, tid);
#pragma unroll
            for (int g = 0; g < (16 >> A2); g++) dif_shift_l4<A2>(v + g * (1 << A2), x + g * (1 << A2));
            if constexpr (G::J >= 3) {
                exchange2_l4<G, A2, G::POS2, A3, 0>(x, v, lds, (const gl_w4 *)twr2, j0inv, tid);
#pragma unroll
                for (int g = 0; g < (16 >> A3); g++) dif_shift_l4<A3>(v + g * (1 << A3), x + g * (1 << A3));
            }
        } else {
#pragma unroll
        for (int g = 0; g < (16 >> A1); g++) dif_shift<A1>(v + g * (1 << A1));
        exchange2<G, A1, G::POS1, A2, G::POS2, TWR_LDS ? 0 : 12 - L, LEAN>(v, lds, TWR_LDS ? twr1 : a.tws, j0inv, tid);
#pragma unroll
        for (int g = 0; g < (16 >> A2); g++) dif_shift<A2>(v + g * (1 << A2));
        if constexpr (G::J >= 3) {
            exchange2<G, A2, G::POS2, A3, 0, TWR_LDS ? 0 : 12 - (A2 + A3), LEAN>(v, lds, TWR_LDS ? twr2 : a.tws, j0inv, tid);
#pragma unroll
            for (int g = 0; g < (16 >> A3); g++) dif_shift<A3>(v + g * (1 << A3));
        }
        }
#pragma unroll
        for (int g = 0; g < GRJ; g++) {
            const int gamma = g * NT + tid;
            const int t = gamma & (T - 1), o = gamma >> LOGT;
            const int klow = G::kof(o << AJ);
            if constexpr (TW1) {
                const int jr = j0inv & ((1 << AJ) - 1);
                // (the field at bit 0: the swizzle takes k_j only on the tiles of 32 columns; the limb form keeps lpos -- its registers are counted)
                const int lane = G::wr_lane(o, t, 0, AJ);
#pragma unroll
                for (int i = 0; i < (1 << AJ); i++) {
                    const int kj = (jr * i) & ((1 << AJ) - 1);
                    if constexpr (LIMB) lds[G::lpos(slot_of(o, kj, 0, AJ), t)] = gl_l4_canon(x[g * (1 << AJ) + brev(i, AJ)]);
                    else tile_store_at(lane ^ G::wr_uni(kj, 0, AJ), v[g * (1 << AJ) + brev(i, AJ)]);
                }
            } else if constexpr (TRANSPOSE) {
                const int jr = j0inv & ((1 << AJ) - 1);  // odd, < 2^AJ: floor(jr*i/2^AJ) steps by 0 or 1
                u64 w = gl_mul(twl_c[g], twh_c[g]);
                const u64 hj = gl_mul(twl_c[GRJ], twh_c[GRJ]);
                const u64 hjd = gl_mul(hj, gl_mul(twl_c[GRJ + 1], twh_c[GRJ + 1]));
#pragma unroll
                for (int i = 0; i < (1 << AJ); i++) {
                    const int p = brev(i, AJ);
                    const int kj = (jr * i) & ((1 << AJ) - 1);
                    u64 x = v[g * (1 << AJ) + p];
                    if (i + 1 < (1 << AJ)) {
                        const bool wrap = ((jr * (i + 1)) >> AJ) != ((jr * i) >> AJ);  // wave-uniform
                        u64 wn = w;
                        gl_mul2(x, w, wn, wrap ? hjd : hj);
                        w = wn;
                    } else {
                        x = gl_mul1(x, w);
                    }
                    lds[G::lpos(slot_of(o, kj, 0, AJ), t)] = x;
                }
            } else {
                // store address = (uniform: s-block + the tile's first column + k-step)  +  (lane: klow rows + t), as for the loads
                u64 *const sbase = dst + (s << (logP + L)) + (u0 & ((1ULL << logP) - 1));
                const u32 lane_sb = (((u32)klow << logP) + (u32)t) << 3;
                const u64 lane_se = ((u64)klow << logP) + (u64)t;
                u64 cw = 1;
                if constexpr (MODE == 2) cw = gl_mul(twl_c[TPL], twh_c[TPL]);  // shift^c, c < Pprev
#pragma unroll
                for (int p = 0; p < (1 << AJ); p += 2) {
                    const int kja = (j0inv * brev(p, AJ)) & ((1 << AJ) - 1), kjb = (j0inv * brev(p + 1, AJ)) & ((1 << AJ) - 1);
                    const int ka = klow + (kja << (L - AJ)), kb = klow + (kjb << (L - AJ));
                    u64 xa, xb;
                    if constexpr (LIMB) {
                        if constexpr (out_tab) {
                            xa = gl_l4_mul(x[g * (1 << AJ) + p], w4_load((const gl_w4 *)tab + ka));
                            xb = gl_l4_mul(x[g * (1 << AJ) + p + 1], w4_load((const gl_w4 *)tab + kb));
                        } else {
                            xa = gl_l4_canon(x[g * (1 << AJ) + p]);
                            xb = gl_l4_canon(x[g * (1 << AJ) + p + 1]);
                        }
                    } else {
                        xa = v[g * (1 << AJ) + p];
                        xb = v[g * (1 << AJ) + p + 1];
                        if constexpr (out_tab) gl_mul2(xa, tab[ka], xb, tab[kb]);
                    }
                    if constexpr (MODE == 2) gl_mul2(xa, cw, xb, cw);
                    // uniform, and through sgpr_opaque a scalar base of its own: the store takes it beside the 32-bit lane offset
                    zp_gu64 *const ua = (zp_gu64 *)sgpr_opaque<LEAN>((u64)(sbase + ((u64)(kja << (L - AJ)) << logP)));
                    zp_gu64 *const ub = (zp_gu64 *)sgpr_opaque<LEAN>((u64)(sbase + ((u64)(kjb << (L - AJ)) << logP)));
                    zp_gu64 *pa, *pb;
                    if constexpr (small_n) { pa = (zp_gu64 *)((zp_gchar *)ua + lane_sb); pb = (zp_gu64 *)((zp_gchar *)ub + lane_sb); }
                    else { pa = ua + lane_se; pb = ub + lane_se; }
                    if constexpr (LOGT < 4) {
                        *pa = xa;
                        *pb = xb;
                    } else {
                        ZP_STG(pa, xa);
                        ZP_STG(pb, xb);
                    }
                }
            }
        }
        if constexpr (TW1) {
            table_copy_out<G, LEAN>(v, a.tw1 + (u0 << L), dst + (u0 << L), tid);
        } else if constexpr (TRANSPOSE) {
            lds_barrier();
            u64 *blk = dst + (u0 << L);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int idx = i * NT + tid;
                const int t2 = idx >> L, k = idx & ((1 << L) - 1);
                ZP_STG(&blk[idx], lds[G::lpos(G::sigma_of_k(k), t2)]);
            }
        }
        if (more) {
            if constexpr (CAN_IN) {
                // every lane is past this tile's exchange barrier, so past its reads of itl: the next tile's entries go in
                if constexpr (in_tab) {
#pragma unroll
                    for (int j = 0; j < TPL; j++)
                        if (tid + j * NT < R) itl[tid + j * NT] = twl_n[j];
                }
            }
            lds_barrier();  // LDS (tile + tables) is reused by the next tile
        }
    };
    if constexpr (!LEAN) {
        // one tile per trip, and the hand-over
#pragma clang loop unroll(disable)
        for (int it = 0; it < tiles_per_wg; it++) {
            tile_step(v, twl_c, twh_c, vn, twl_n, twh_n, it);
            if (it + 1 < tiles_per_wg) {
#pragma unroll
                for (int i = 0; i < 16; i++) v[i] = vn[i];
#pragma unroll
                for (int i = 0; i < NTW; i++) { twl_c[i] = twl_n[i]; twh_c[i] = twh_n[i]; }
            }
        }
    } else {
        // two tiles per trip; an odd count (1 included) leaves after the first
#pragma clang loop unroll(disable)
        for (int it = 0;; it += 2) {
            tile_step(v, twl_c, twh_c, vn, twl_n, twh_n, it);
            if (it + 1 >= tiles_per_wg) break;
            tile_step(vn, twl_n, twh_n, v, twl_c, twh_c, it + 1);
            if (it + 2 >= tiles_per_wg) break;
        }
    }
}


// ---- the seam of an extension (blow-up 2): the LAST pass of the inverse transform and the FIRST pass of the zero-padded forward transform
// in one kernel.  The inverse's last radix-256 pass delivers a tile of coefficients { k N/256 + c : k < 256, c in 16 consecutive } -- and
// the forward transform of 2N points starts with a radix-256 pass over { r 2N/256 + u : r < 128 } (rows 128.. are the zero padding): the
// same index set, k = 2 r + (u >> log(N/256)), c = u mod N/256.  So one inverse tile IS two forward tiles (k even / k odd), and the
// scaled coefficients never have to leave the CU: they are handed over through the tile's LDS (the 128 non-zero rows of both forward
// tiles = the 4 096 elements of the inverse tile), each lane picks up its 2 x 8 non-zero inputs, and the two forward tiles go through
// the first-pass body (first butterfly level of a half-zero register file: a copy and a shift).  Per column this saves the write and
// the read of the coefficient buffer (16 N of 136 N bytes; 8 N when the caller wants the coefficients: `coef`), and one launch.
// Inverse side = ntt_pass2_kernel<4,4,0,4,false,false,2,TAB_FIXED>, forward side = <4,4,0,4,true,true,3,TAB_NONE>: the same values, bit for bit.
struct SeamArgs {
    const u64 *in;          // input of the inverse transform's last pass, columns of N
    u64 *out;               // output of the forward transform's first pass, columns of 2N
    u64 *coef;              // scaled coefficients c_i shift^i, columns of N (may be null)
    const u64 *tws_i, *tws_f;   // w_4096^e of the inverse / the forward plan
    const u64 *tw1;         // the forward plan's first-pass table, [u * 256 + k]
    const u64 *csl, *csh;   // coset table of the inverse transform's post-scale
    u64 scale;              // 1 / N
    int logn, cslb, j0inv_i, j0inv_f, ncols;
};
// No prefetch of the next tile (unlike ntt_pass2_kernel): a tile is three bodies of integer work per load, the other workgroups of the CU cover
// the one exposed load latency, and the 32 registers it would hold keep the kernel at 128 VGPRs = four waves per SIMD (with them it spilled).
// (The limb form of gl_limb.hpp was tried here too, this kernel being bound by its integer work: 64 more live registers -- 0.77 ms at two waves
// per SIMD, 1.37 ms spilling at three, against 0.70 ms: profiles/r4_lde_seam_ab.txt.  Removed.)
__global__ void __launch_bounds__(256, 4) lde_seam_kernel(SeamArgs a, int tiles_per_wg) {
    using G = Geo<4, 4, 0, 4>;
    constexpr int L = 8, R = 256, T = 16, LOGT = 4;
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    u64 *tab = lds + R * T;        // 1/N shift^(k N/256)
    u64 *twr_i = tab + R;          // inter-round twiddles of the inverse pass
    u64 *twr_f = twr_i + R;        // ... of the forward pass
    const u64 x8 = blockIdx.x & 7u, jj = blockIdx.x >> 3;
    const u64 col = jj % (u64)a.ncols, wg = (jj / (u64)a.ncols) * 8 + x8;
    const int logNR = a.logn - L;                      // log(N / 256): the inverse pass's Pprev, and the split of u
    const u64 N = 1ULL << a.logn;
    const u64 *src = a.in + col * N;
    u64 *dst = a.out + col * (2 * N);
    u64 *cdst = a.coef ? a.coef + col * N : nullptr;
    u64 v[16];
    u64 cw_c[2];                                       // raw halves of shift^c for this lane's column c
    auto fetch_tile = [&](u64 *r, u64 *cwr, u64 u0, int tid) {
        const int t = tid & (T - 1), o = tid >> LOGT;
        const u32 slot0 = (u32)slot_of(o, 0, G::POS1, 4);
        const u32 lane_bytes = (((u32)slot0 << logNR) + (u32)t) << 3;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const u64 *rowp = src + (((u64)j << G::POS1) << logNR) + u0;      // wave-uniform
            r[j] = ZP_LDG((const u64 *)((const char *)rowp + lane_bytes));
        }
        const u64 c = u0 + (u64)t;
        cwr[0] = a.csl[c & ((1ULL << a.cslb) - 1)];
        cwr[1] = a.csh[c >> a.cslb];
    };
    const u64 tile0 = wg * tiles_per_wg;
    {
        const int tid0 = threadIdx.x;
        twr_i[tid0] = a.tws_i[tid0 << (12 - L)];
        twr_f[tid0] = a.tws_f[tid0 << (12 - L)];
        const u64 ek = (u64)tid0 << logNR;
        tab[tid0] = gl_mul(a.scale, gl_mul(a.csl[ek & ((1ULL << a.cslb) - 1)], a.csh[ek >> a.cslb]));
    }
    lds_barrier();
#pragma clang loop unroll(disable)
    for (int it = 0; it < tiles_per_wg; it++) {
        const u64 u0 = (tile0 + it) << LOGT;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        fetch_tile(v, cw_c, u0, tid);
        const int t = tid & (T - 1), o = tid >> LOGT;
        // ---- inverse transform, last pass (radix 256, plain last pass of the plan: no inter-pass twiddle; 1/N and the coset power)
        dif_shift<4>(v);
        exchange2<G, 4, G::POS1, 4, G::POS2, 0>(v, lds, twr_i, a.j0inv_i, tid);
        dif_shift<4>(v);
        const u64 cw = gl_mul(cw_c[0], cw_c[1]);       // shift^c
        lds_barrier();                                  // the exchange's reads are done: the tile becomes the hand-over buffer
#pragma unroll
        for (int p = 0; p < 16; p += 2) {
            const int kja = (a.j0inv_i * brev(p, 4)) & 15, kjb = (a.j0inv_i * brev(p + 1, 4)) & 15;
            const int ka = o + (kja << 4), kb = o + (kjb << 4);           // klow = o for <4,4,0>
            u64 xa = v[p], xb = v[p + 1];
            gl_mul2(xa, tab[ka], xb, tab[kb]);
            gl_mul2(xa, cw, xb, cw);
            if (cdst) {
                ZP_STG((u64 *)((char *)(cdst + ((u64)ka << logNR) + u0) + (t << 3)), xa);
                ZP_STG((u64 *)((char *)(cdst + ((u64)kb << logNR) + u0) + (t << 3)), xb);
            }
            // forward tile par = k & 1, row r = k >> 1: [par][r][t]
            lds[(((ka & 1) << 7) + (ka >> 1)) * T + t] = xa;
            lds[(((kb & 1) << 7) + (kb >> 1)) * T + t] = xb;
        }
        lds_barrier();
        // this lane's non-zero inputs of both forward tiles: rows r = 16 j + o, j < 8 (rows 128.. are the padding)
        u64 f1[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            v[j] = lds[((j << 4) + o) * T + t];
            f1[j] = lds[(128 + (j << 4) + o) * T + t];
        }
        lds_barrier();
        // ---- forward transform of 2N points, first pass, tiles u0f = par * N/256 + u0
#pragma unroll 1
        for (int par = 0; par < 2; par++) {
            if (par) {
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = f1[j];
            }
            // first butterfly level of a half-zero register file: (x + 0, (x - 0) 2^(12 j)); then two radix-8 halves
#pragma unroll
            for (int j = 1; j < 8; j++) v[8 + j] = mul_c16(j, v[j]);
            v[8] = v[0];
            dif_shift<3>(v);
            dif_shift<3>(v + 8);
            exchange2<G, 4, G::POS1, 4, G::POS2, 0>(v, lds, twr_f, a.j0inv_f, tid);
            dif_shift<4>(v);
            {
                const int jr = a.j0inv_f & 15;
                const int lane = G::wr_lane(o, t, 0, 4);
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int kj = (jr * i) & 15;
                    tile_store_at(lane ^ G::wr_uni(kj, 0, 4), v[brev(i, 4)]);
                }
            }
            const u64 u0f = ((u64)par << logNR) + u0;
            table_copy_out<G, true>(v, a.tw1 + (u0f << L), dst + (u0f << L), tid);
            lds_barrier();      // the tile is reused by the second forward tile / the next inverse tile
        }
    }
}

// ---- small transforms (N <= 4096): one workgroup per column, radix-2 DIF stages in LDS
struct SmallArgs {
    const u64 *in;
    u64 *out;
    u64 in_cs, out_cs, in_valid;
    const u64 *tws;
    const u64 *csl, *csh;
    u64 scale;
    int logn, cslb, flags;
};

// one DIF stage of half 2^LH inside a wave: lane l holds element l of a 64-element block; the lane with bit LH clear keeps the sum, its
// partner the twiddled difference.  Every lane walks both sides (the wave executes the sum and the product under complementary masks):
// twice the arithmetic per element of the LDS form, no LDS traffic and no barrier
template <int LH>
__device__ __forceinline__ u64 wave_stage(u64 x, int lane, const u64 *tws) {
    const u64 y = lane_xor<LH>(x);
    const int i = lane & ((1 << LH) - 1);
    if (!((lane >> LH) & 1)) return gl_add(x, y);
    const u64 d = gl_sub(y, x);
    return i ? gl_mul(d, tws[(u64)i << (12 - (LH + 1))]) : d;
}

// WAVE: the last min(logn, 6) stages (halves 32 .. 1) run inside a wave on lane exchanges (zp_set_tuning "ntt_small_wave"; the A/B against
// the all-LDS form is profiles/r5_dpp_ab.txt)
template <bool WAVE>
__global__ void __launch_bounds__(256) ntt_small_kernel(SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int tid = threadIdx.x;
    const int n = 1 << a.logn;
    const u64 *src = a.in + (u64)blockIdx.x * a.in_cs;
    u64 *dst = a.out + (u64)blockIdx.x * a.out_cs;
    for (int i = tid; i < n; i += 256) lds[i] = (u64)i < a.in_valid ? src[i] : 0ULL;
    __syncthreads();
    const int lds_stages = WAVE ? (a.logn > 6 ? a.logn - 6 : 0) : a.logn;
    for (int s = 0; s < lds_stages; s++) {
        const int lh = a.logn - 1 - s;  // log2(half)
        const int half = 1 << lh;
        for (int b = tid; b < (n >> 1); b += 256) {
            const int i = b & (half - 1);
            const int i0 = ((b >> lh) << (lh + 1)) + i, i1 = i0 + half;
            u64 x = lds[i0], y = lds[i1];
            lds[i0] = gl_add(x, y);
            u64 d = gl_sub(x, y);
            lds[i1] = i ? gl_mul(d, a.tws[(u64)i << (12 - (lh + 1))]) : d;
        }
        __syncthreads();
    }
    if constexpr (WAVE) {
        const int lane = tid & 63;
        for (int base = (tid >> 6) << 6; base < n; base += 256) {       // (n < 64: one partial block; lanes >= n carry zeros nobody stores)
            u64 x = base + lane < n ? lds[base + lane] : 0ULL;
            const int top = a.logn < 6 ? a.logn : 6;                    // stages with half 2^(top-1) .. 1
            if (top >= 6) x = wave_stage<5>(x, lane, a.tws);
            if (top >= 5) x = wave_stage<4>(x, lane, a.tws);
            if (top >= 4) x = wave_stage<3>(x, lane, a.tws);
            if (top >= 3) x = wave_stage<2>(x, lane, a.tws);
            if (top >= 2) x = wave_stage<1>(x, lane, a.tws);
            if (top >= 1) x = wave_stage<0>(x, lane, a.tws);
            const int i = base + lane;
            if (i < n) {
                const int k = brev(i, a.logn);
                if (a.flags & 2) x = gl_mul(x, a.scale);
                if (a.flags & 4) x = gl_mul(x, tw_lookup(a.csl, a.csh, a.cslb, (u64)k));
                dst[k] = x;
            }
        }
        return;
    }
    for (int i = tid; i < n; i += 256) {
        const int k = brev(i, a.logn);
        u64 x = lds[i];
        if (a.flags & 2) x = gl_mul(x, a.scale);
        if (a.flags & 4) x = gl_mul(x, tw_lookup(a.csl, a.csh, a.cslb, (u64)k));
        dst[k] = x;
    }
}

// out[i] = in[i] * shift^i  (coefficients -> coset-scaled coefficients), 2 elements per thread
__global__ void __launch_bounds__(256) coset_scale_kernel(const u64 *in, u64 *out, u64 n, const u64 *lo,
                                                         const u64 *hi, int lb) {
    const u64 col = blockIdx.y;
    const u64 i = ((u64)blockIdx.x * 256 + threadIdx.x);
    if (i < n) out[col * n + i] = gl_mul(in[col * n + i], tw_lookup(lo, hi, lb, i));
}

// four-step NTT of one column split over GPUs: between the two local transforms every element of the
// N2/G x N1 block is multiplied by w_N^(i2 * k1):  rows[r][k] *= w_N^((row0 + r) * k)
__global__ void __launch_bounds__(256) twiddle_rows_kernel(u64 *rows, int logn_row, u64 total, u64 row0, u64 nmask,
                                                           const u64 *lo, const u64 *hi, int lb) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u64 r = i >> logn_row, k = i & ((1ULL << logn_row) - 1);
    const u64 e = ((row0 + r) * k) & nmask;
    rows[i] = gl_mul(rows[i], tw_lookup(lo, hi, lb, e));
}

// the table of the transposing pass (MODE 3): out[u * R + k] = w^(u k mod N), N = 2^logn, R = 2^L
__global__ void __launch_bounds__(256) tw1_fill_kernel(u64 *out, int logn, int L, const u64 *lo, const u64 *hi, int lb) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >> logn) return;
    const u64 u = i >> L, k = i & ((1ULL << L) - 1);
    out[i] = tw_lookup(lo, hi, lb, (u * k) & ((1ULL << logn) - 1));
}

// the input-side table of a last pass (PassArgs::itab): out[k * R + r] = pre * w^(Pp k r mod N), k < Rprev, r < R = 2^L, Pp = 2^logPp
__global__ void __launch_bounds__(256) itab_fill_kernel(u64 *out, u64 total, int logn, int L, int logPp, u64 pre, const u64 *lo, const u64 *hi, int lb) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u64 k = i >> L, r = i & ((1ULL << L) - 1);
    out[i] = gl_mul(pre, tw_lookup(lo, hi, lb, ((k * r) << logPp) & ((1ULL << logn) - 1)));
}

using PassKernel = void (*)(PassArgs, int);

// The instantiation a launch takes.  First passes: the table form (MODE 3, never BIG, two-round shapes only) with or without limb
// butterflies, or the per-lane chain (MODE 1); either reads a zero-padded input or a full one.  Later passes: `mode` 0..2 with the table
// that run_one_pass gives that mode (the list below is all it can ask for), limb or not.  Null: not built.
template <int A1, int A2, int A3, int LOGT, bool BIG, bool LIMB>
PassKernel pick_later_pass(int mode, int tab) {
    if (mode == 2) return tab == TAB_FIXED ? ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 2, TAB_FIXED, BIG, LIMB> : nullptr;   // coset powers, with or without 1/N
    if (mode == 1)
        return tab == TAB_TILE    ? ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 1, TAB_TILE, BIG, LIMB>    // a middle pass with its inter-pass twiddle
               : tab == TAB_FIXED ? ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 1, TAB_FIXED, BIG, LIMB>   // a last pass that multiplies by 1/N
               : tab == TAB_NONE  ? ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 1, TAB_NONE, BIG, LIMB>    // the plain pass before a last pass with TAB_IN
                                  : nullptr;
    if constexpr (A1 + A2 + A3 <= 9) {
        if (tab == TAB_IN) return ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 0, TAB_IN, BIG, LIMB>;
    }
    return tab == TAB_NONE ? ntt_pass2_kernel<A1, A2, A3, LOGT, false, false, 0, TAB_NONE, BIG, LIMB> : nullptr;
}
template <int A1, int A2, int A3, int LOGT, bool BIG>
PassKernel pick_pass_kernel(bool transpose, bool table, bool padded, int mode, int tab, bool limb) {
    constexpr bool CAN_TABLE = !BIG && A3 == 0, CAN_LIMB = !BIG && A1 + A2 + A3 <= 8;
    if constexpr (CAN_TABLE) {
        if (table && limb) return padded ? ntt_pass2_kernel<A1, A2, A3, LOGT, true, true, 3, TAB_NONE, false, CAN_LIMB> : ntt_pass2_kernel<A1, A2, A3, LOGT, true, false, 3, TAB_NONE, false, CAN_LIMB>;
        if (table) return padded ? ntt_pass2_kernel<A1, A2, A3, LOGT, true, true, 3, TAB_NONE, false> : ntt_pass2_kernel<A1, A2, A3, LOGT, true, false, 3, TAB_NONE, false>;
    }
    if (transpose) return padded ? ntt_pass2_kernel<A1, A2, A3, LOGT, true, true, 1, TAB_NONE, BIG> : ntt_pass2_kernel<A1, A2, A3, LOGT, true, false, 1, TAB_NONE, BIG>;
    return limb ? pick_later_pass<A1, A2, A3, LOGT, BIG, CAN_LIMB>(mode, tab) : pick_later_pass<A1, A2, A3, LOGT, BIG, false>(mode, tab);
}

template <int A1, int A2, int A3, int LOGT, bool BIG = false>
int32_t launch_pass2(zp_ctx *ctx, PassArgs a, bool transpose, int W) {
    using G = Geo<A1, A2, A3, LOGT>;
    const u64 tiles = (1ULL << (a.logn - G::L)) >> LOGT;
    // tiles per workgroup: a power of two that divides the tile count and (passes >= 2) keeps a
    // workgroup inside one s-block only by construction of the table per tile (no constraint)
    int tpw = ctx->tune_tpw;
    while (tpw > 1 && (tiles % tpw != 0 || tiles / tpw * (u64)W < (u64)ctx->num_cu * 4)) tpw >>= 1;
    dim3 grid((unsigned)(tiles / tpw), (unsigned)W), block(G::NT);
    // table form of a first pass: a one-dimensional grid, XCD-ordered (ntt_pass2_kernel, MODE 3)
    const bool table = !BIG && A3 == 0 && transpose && a.tw1 && (grid.x & 7u) == 0;
    // MODE of a later pass: 2 = coset post-scale, 1 = a middle pass or one with a table on the output side (inter-pass twiddle or 1/N),
    // 0 = a last pass that stores what its rounds deliver
    const int mode = transpose ? 0 : (a.flags & 4) ? 2 : (a.flags & 11) ? 1 : 0;
    // limb-form butterflies (gl_limb.hpp; knob ntt_limb): every pass with LDS twiddle copies except a first pass without its table
    // (radix 2^9 and up: tiles of 64 / 128 KiB leave no room for the 32-byte table records)
    const bool limb = !BIG && G::L <= 8 && ctx->tune_ntt_limb != 0 && (!transpose || table);
    // tile + (per-tile table: non-transposing passes with a multiplication) + (LDS copies of the inter-round twiddles, L <= 10)
    const size_t rec = limb ? 4 : 1;
    // + (the tile's input-side factors: a last pass that takes them)
    const size_t shmem = ((size_t)G::R * G::T + (mode >= 1 ? G::R * rec : 0) + (G::L <= 10 ? (G::R + (1 << (A2 + A3))) * rec : 0) + (a.itab ? G::R : 0)) * sizeof(u64);
    // ... and the table of that pass, a template argument like the mode: the tile loop of a kernel holds its own case only
    const int tab = transpose ? TAB_NONE : a.itab ? TAB_IN : (a.flags & 1) ? TAB_TILE : (a.flags & 6) ? TAB_FIXED : TAB_NONE;
    const PassKernel k = pick_pass_kernel<A1, A2, A3, LOGT, BIG>(transpose, table, a.in_valid != (1ULL << a.logn), mode, tab, limb);
    if (!k) {
        ctx->err = "pass kernel not built for this combination of output scaling and tables";
        return ZP_ERR_UNSUPPORTED;
    }
    if (shmem > 65536) ZP_HIP(ctx, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    if (table) {
        a.ncols = W;
        grid = dim3(grid.x * (unsigned)W);
    }
    hipLaunchKernelGGL(k, grid, block, shmem, ctx->stream, a, tpw);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}

constexpr int shape_key(int A1, int A2, int A3, int logT, bool big) { return (((A1 * 8 + A2) * 8 + A3) * 8 + logT) * 2 + big; }

// one case per shape that is built: the list of what zpi_pass_shape can return
int32_t dispatch_pass(zp_ctx *ctx, const NttPass &p, const PassArgs &a, bool transpose, int W) {
    const bool big = a.logn > 28;
    const NttPassShape s = zpi_pass_shape(ctx, p.L, big, transpose, (a.flags & 7) != 0 || a.itab);
#define ZP_PASS_SHAPE(A1, A2, A3, LOGT, BIG) case shape_key(A1, A2, A3, LOGT, BIG): return launch_pass2<A1, A2, A3, LOGT, BIG>(ctx, a, transpose, W)
    switch (shape_key(s.A1, s.A2, s.A3, s.logT, big)) {
        ZP_PASS_SHAPE(3, 2, 0, 5, false);
        ZP_PASS_SHAPE(3, 3, 0, 5, false);
        ZP_PASS_SHAPE(4, 3, 0, 5, false);
        ZP_PASS_SHAPE(4, 3, 0, 5, true);
        ZP_PASS_SHAPE(4, 4, 0, 4, false);
        ZP_PASS_SHAPE(4, 4, 0, 4, true);
        ZP_PASS_SHAPE(4, 4, 0, 5, false);
        ZP_PASS_SHAPE(3, 3, 3, 4, false);
        ZP_PASS_SHAPE(3, 3, 3, 5, false);
        ZP_PASS_SHAPE(4, 3, 3, 4, false);
        ZP_PASS_SHAPE(4, 4, 3, 3, false);
        ZP_PASS_SHAPE(4, 4, 4, 1, false);
        ZP_PASS_SHAPE(4, 4, 4, 2, false);
        default: ctx->err = big ? "pass radix not built for transforms above 2^28 rows" : "unsupported pass radix"; return ZP_ERR_UNSUPPORTED;
    }
#undef ZP_PASS_SHAPE
}

// brackets one launch with HIP events on the ctx stream when profiling is on (zp_get_pass_timings).  radix_log: L of a pass,
// -L of a first pass, 88 of the seam kernel (inverse radix 2^8 + forward radix 2^8)
struct PassTimer {
    zp_ctx *ctx;
    zp_ctx::PassEv ev;
    bool on;
    PassTimer(zp_ctx *c, int radix_log) : ctx(c), on(c->profiling) {
        ev.radix_log = radix_log;
        on = on && hipEventCreate(&ev.a) == hipSuccess && hipEventCreate(&ev.b) == hipSuccess && hipEventRecord(ev.a, ctx->stream) == hipSuccess;
    }
    ~PassTimer() {
        if (on && hipEventRecord(ev.b, ctx->stream) == hipSuccess) ctx->pass_events.push_back(ev);
    }
};

// what the last pass (or the small kernel) does to its outputs: 1/N of an inverse transform, the coset table of an LDE
template <typename Args>
void set_output_scaling(Args &a, bool inverse, const CosetTable *post_scale) {
    if (inverse) a.flags |= 2;
    if (post_scale) {
        a.flags |= 4;
        a.csl = post_scale->d_lo;
        a.csh = post_scale->d_hi;
        a.cslb = post_scale->lb;
    }
}

// columns per launch: chunks such that a ping-pong scratch buffer (and the LDE's scaled-coefficient buffer) stays <= 2 GiB.  2^28 elements
// per launch since round 4 (profiles/r4_chunk_sweep.txt: NTT 2^20 .. 2^25 0-3 % faster than at 2^27, the first pass's shared twiddle table
// now serving 16 columns of a tile; 2^29 adds nothing.  Round 2, before that table, measured the opposite: profiles/r2_chunk_sweep.txt)
int chunk_columns(const zp_ctx *ctx, int logn, int W) {
    const int wc = (int)((1ULL << (ctx->tune_ntt_chunk_log > 0 ? ctx->tune_ntt_chunk_log : 28)) >> logn);
    return wc < 1 ? 1 : wc > W ? W : wc;
}

}  // namespace

NttPassShape zpi_pass_shape(const zp_ctx *ctx, int L, bool big, bool transpose, bool multiplies) {
    // L = 5 .. 12 at the default knobs.  Radix 2^10 .. 2^12: 1024-thread workgroups on 128 KiB tiles, two-pass plans up to 2^20 / 2^22 / 2^24
    // (runs of 128 / 64 / 32 bytes)
    static const NttPassShape by_l[8] = {{3, 2, 0, 5}, {3, 3, 0, 5}, {4, 3, 0, 5}, {4, 4, 0, 4}, {3, 3, 3, 4}, {4, 3, 3, 4}, {4, 4, 3, 3}, {4, 4, 4, 2}};
    // 64-bit lane offsets (big): only the shapes the default plan uses above 2^28 rows (digits 7 and 8), whatever the knobs
    if (L < 5 || L > 12 || (big && L != 7 && L != 8)) return {0, 0, 0, 0};
    NttPassShape s = by_l[L - 5];
    if (big) return s;
    if ((L == 8 && ctx->tune_logt != 4) || (L == 9 && ctx->tune_logt9 != 4)) s.logT = 5;
    // (round 6, review item 4: knob ntt_logt12 = 1 -- 512-thread workgroups on 64-KiB tiles of 2 columns, TWO workgroups per CU, 16-byte runs;
    //  a pass with a per-tile twiddle table needs 32 KiB more and stays on the 4-column tile)
    if (L == 12 && ctx->tune_logt12 == 1 && (transpose || !multiplies)) s.logT = 1;
    return s;
}

NttPassShape zpi_plan_pass_shape(const zp_ctx *ctx, const NttPlan *pl, int i) {
    return zpi_pass_shape(ctx, pl->pass[i].L, pl->logn > 28, i == 0, i + 1 < pl->npass || pl->inverse);
}

// two-level table of pre * base^e, e < 2^logn:  lo[e & (2^lb - 1)] * hi[e >> lb]
static int32_t upload_power_table(zp_ctx *ctx, int logn, u64 base, u64 pre, int *lb, u64 **d_lo, u64 **d_hi) {
    *lb = (logn + 1) / 2;
    std::vector<u64> lo(1ULL << *lb), hi(1ULL << (logn - *lb));
    lo[0] = pre;
    u64 sp = 1;
    for (size_t i = 1; i < lo.size(); i++) {
        sp = gl_mul(sp, base);
        lo[i] = gl_mul(pre, sp);
    }
    const u64 sl = gl_mul(sp, base);  // base^(2^lb)
    hi[0] = 1;
    for (size_t i = 1; i < hi.size(); i++) hi[i] = gl_mul(hi[i - 1], sl);
    ZP_TRY(zpi_upload(ctx, lo, d_lo));
    return zpi_upload(ctx, hi, d_hi);
}

// role (the two sides of an extension's seam, zpi_lde): 0 = the default plan; 1 = a plan that ENDS in a radix-256 pass (the inverse
// transform in front of lde_seam_kernel); 2 = one that STARTS with a radix-256 pass (the forward transform behind it).  The digit 8 is
// fixed, the other logn - 8 bits are split over as few passes as the default plan would use for them, the first of them >= 7 where that
// leaves >= 5 for the rest (a first pass of radix >= 2^7 takes its twiddles from the shared table).  ZP_ERR_UNSUPPORTED when that takes
// more passes than the default plan (the caller then runs the two transforms unfused).
int32_t zpi_get_plan_role(zp_ctx *ctx, int logn, bool inverse, int role, NttPlan **out) {
    const int maxl = (ctx->tune_ntt_maxl >= 6 && ctx->tune_ntt_maxl <= 12) ? ctx->tune_ntt_maxl : 9;
    const int order = ctx->tune_ntt_order;          // 0: auto, 1: larger digits first, 2: larger digits last
    const int key = (((logn * 2 + (inverse ? 1 : 0)) * 16 + maxl) * 4 + (order & 3)) * 4 + (role & 3);
    int rdig[6], nr = 0;
    if (role) {
        const int r = logn - 8, m_default = (logn + maxl - 1) / maxl;
        if (logn <= 12 || r < 5 || maxl != 9) return ZP_ERR_UNSUPPORTED;
        nr = (r + maxl - 1) / maxl;
        if (1 + nr > m_default || nr > 4) return ZP_ERR_UNSUPPORTED;
        int rem = r;
        for (int i = 0; i < nr; i++) {
            int d = (rem + (nr - i) - 1) / (nr - i);                        // balanced, larger first
            if (i == 0 && nr >= 2 && d < 7 && rem - 7 >= 5 * (nr - 1)) d = 7;
            rdig[i] = d;
            rem -= d;
        }
        for (int i = 0; i < nr; i++)
            if (rdig[i] < 5 || rdig[i] > 9) return ZP_ERR_UNSUPPORTED;
    }
    auto it = ctx->plans.find(key);
    if (it != ctx->plans.end()) {
        *out = &it->second;
        return ZP_OK;
    }
    NttPlan pl;
    pl.logn = logn;
    pl.inverse = inverse;
    pl.role = role;
    u64 w = gl_root(ctx->root32, logn);
    u64 w4096 = gl_root(ctx->root32, 12);
    u64 w16 = gl_root(ctx->root32, 4);
    if (inverse) {
        w = gl_inv(w);
        w4096 = gl_inv(w4096);
        w16 = gl_inv(w16);
    }
    pl.ninv = gl_inv((1ULL << logn) % GL_P);
    pl.j0inv = 0;
    for (int j = 1; j < 16; j += 2)
        if (gl_pow(1ULL << 12, (u64)j) == w16)
            for (int ji = 1; ji < 16; ji += 2)
                if (((j * ji) & 15) == 1) pl.j0inv = ji;
    pl.w16[0] = 1;
    for (int i = 1; i < 8; i++) pl.w16[i] = gl_mul(pl.w16[i - 1], w16);
    std::vector<u64> tws(4096);
    tws[0] = 1;
    for (int i = 1; i < 4096; i++) tws[i] = gl_mul(tws[i - 1], w4096);
    ZP_TRY(zpi_upload(ctx, tws, &pl.d_tws));
    int dig[6];
    if (logn > 12 && role) {
        pl.npass = nr + 1;
        for (int i = 0; i < pl.npass; i++) dig[i] = role == 1 ? (i < nr ? rdig[i] : 8) : (i == 0 ? 8 : rdig[i - 1]);
    } else if (logn > 12) {
        const int m = pl.npass = (logn + maxl - 1) / maxl;
        int rem = logn, digits[6];
        for (int i = 0; i < m; i++) {
            digits[i] = (rem + (m - i) - 1) / (m - i);  // balanced, larger digits first
            rem -= digits[i];
        }
        // the transposing first pass pays a per-lane twiddle chain on top of its rounds: a three-round radix-512 digit is
        // cheaper as the (plain) last pass; with digits <= 8 the larger-first order measured 1-4 % faster
        // (profiles/r2_order_sweep.txt)
        const bool last = order == 2 || (order == 0 && digits[0] == 9 && digits[m - 1] < 9);
        for (int i = 0; i < m; i++) dig[i] = last ? digits[m - 1 - i] : digits[i];
    }
    for (int i = 0, logP = 0; i < pl.npass; logP += dig[i++]) pl.pass[i] = {dig[i], logP};
    ZP_TRY(upload_power_table(ctx, logn, w, 1, &pl.lb, &pl.d_twl, &pl.d_twh));   // w^e, e < N (also used by the FRI fold for w_n^-i)
    auto ins = ctx->plans.emplace(key, pl);
    *out = &ins.first->second;
    return ZP_OK;
}

int32_t zpi_get_plan(zp_ctx *ctx, int logn, bool inverse, NttPlan **out) { return zpi_get_plan_role(ctx, logn, inverse, 0, out); }

// pass i of a plan is a two-round radix-256 pass, the one lde_seam_kernel has built in on either side, and not the plan's only pass
static bool is_radix256_pass(const zp_ctx *ctx, const NttPlan *pl, int i) {
    const NttPassShape s = zpi_plan_pass_shape(ctx, pl, i);
    return pl->npass >= 2 && pl->pass[i].L == 8 && s.A1 == 4 && s.A2 == 4 && s.A3 == 0;
}

// the two plans of a fused extension (blow-up 2) of 2^logn-row columns: the default plans where they already meet in radix-256 passes,
// else the seam-role plans (knob lde_seam_plans: 0 = default plans only).  false: no fused path at this size.
static bool seam_plans(zp_ctx *ctx, int logn, NttPlan **pi, NttPlan **pf) {
    auto fits = [ctx](const NttPlan *i, const NttPlan *f) { return is_radix256_pass(ctx, i, i->npass - 1) && is_radix256_pass(ctx, f, 0); };
    if (zpi_get_plan(ctx, logn, true, pi) != ZP_OK || zpi_get_plan(ctx, logn + 1, false, pf) != ZP_OK) return false;
    // measured on one box (profiles/r5_lde_seam_plans_ab.txt): the seam plans win 1-3 % from 2^21 rows on ((7,6,8)+(8,7,7) .. (8,7,8)+(8,8,8)) and LOSE
    // 5-11 % at 2^19 / 2^20, where fixing one digit at 8 leaves radix-32 passes ((6,5,8)+(8,7,5), (7,5,8)+(8,7,6)): default from 2^21 (knob 2: always)
    if (!fits(*pi, *pf) && (ctx->tune_lde_seam_plans == 2 || (ctx->tune_lde_seam_plans == 1 && logn >= 21))) {
        if (!is_radix256_pass(ctx, *pi, (*pi)->npass - 1) && zpi_get_plan_role(ctx, logn, true, 1, pi) != ZP_OK) return false;
        if (!is_radix256_pass(ctx, *pf, 0) && zpi_get_plan_role(ctx, logn + 1, false, 2, pf) != ZP_OK) return false;
    }
    return fits(*pi, *pf);
}

// How zp_lde runs an extension of 2^logn-row columns by 2^logb, with or without a coefficient store.  fused: blow-up 2 with matching
// radix-256 passes on both sides of the seam -- the last pass of `inv` and the first pass of `fwd` run as ONE kernel (lde_seam_kernel) on
// `tpw` inverse tiles per workgroup, and the scaled coefficients never travel.  Else the two transforms run one after the other.
// Measured (profiles/r4_lde_seam_ab.txt, 2^24 x 32): 19.5 -> 18.7 ms without the coefficient store -- the fused kernel does three tile
// bodies of integer work for three units of traffic and is bound by the former (0.70 ms against 0.73 ms for the two launches it replaces,
// and the forward transform's remaining passes run on fewer launches): a pass of this library is BALANCED between its integer work and its
// traffic, so taking away either alone buys little.  On by default where the caller does not want the coefficients (knob lde_seam: 0 never,
// 1 default, 2 always).  (What this cannot know: the forward plan's table may fail to allocate; zpi_lde then takes the other path.)
struct LdeRoute { bool fused = false; NttPlan *inv = nullptr, *fwd = nullptr; int tpw = 0; };
static LdeRoute lde_route(zp_ctx *ctx, int logn, int logb, bool want_coef) {
    LdeRoute r;
    r.tpw = (ctx->tune_seam_tpw == 1 || ctx->tune_seam_tpw == 4) ? ctx->tune_seam_tpw : 2;     // a power of two: divides the tile count
    r.fused = logb == 1 && (ctx->tune_lde_seam == 2 || (ctx->tune_lde_seam == 1 && !want_coef)) &&
              zpi_pass_shape(ctx, 8, false, true, true).logT == 4 &&                              // the seam kernel's tiles are 16 columns wide
              logn >= 16 && logn + 1 <= 28 && logn + 1 <= ctx->tune_ntt_tw1 && seam_plans(ctx, logn, &r.inv, &r.fwd) &&
              ((((1ULL << logn) >> 12) / r.tpw) & 7u) == 0;                                       // its grid is XCD-ordered: a multiple of 8 workgroups per column
    return r;
}

int32_t zpi_get_coset(zp_ctx *ctx, int logn, u64 shift, u64 pre, CosetTable **out) {
    for (auto &c : ctx->cosets)
        if (c.logn == logn && c.shift == shift && c.pre == pre) {
            *out = &c;
            return ZP_OK;
        }
    CosetTable c;
    c.logn = logn;
    c.shift = shift;
    c.pre = pre;
    ZP_TRY(upload_power_table(ctx, logn, shift, pre, &c.lb, &c.d_lo, &c.d_hi));
    ctx->cosets.push_back(c);
    *out = &ctx->cosets.back();
    return ZP_OK;
}

bool zpi_plan_uses_tw1(const zp_ctx *ctx, const NttPlan *pl) {
    const int logn = pl->logn;
    return pl->npass >= 1 && !pl->tw1_unavailable && logn > 12 && logn <= ctx->tune_ntt_tw1 && logn <= 28 && zpi_plan_pass_shape(ctx, pl, 0).A3 == 0 &&
           pl->pass[0].L >= 7;
}

// The last pass of a plan of three passes or more multiplies its INPUT by the inter-pass twiddle of the pass before it (and by 1/N of an
// inverse plan), which then runs plain: ntt_pass2_kernel, a.itab.  Rprev x R entries per plan (512 KiB at 2^24 rows), capped at 2 MiB;
// radix 2^10 and up keep the output-side table of the pass before (their tiles leave the LDS no room that is worth a new shape rule).
bool zpi_plan_uses_itab(const NttPlan *pl) {
    const int m = pl->npass;
    // (role 1: a plan that only ever runs in front of the seam kernel, whose built-in last pass takes no such table)
    return m >= 3 && pl->role != 1 && !pl->itab_unavailable && pl->pass[m - 1].L <= 9 && pl->pass[m - 2].L + pl->pass[m - 1].L <= 18;
}

// pass i of a plan over w columns: cur (column stride cur_cs, in_valid real elements per column) -> nxt (column stride N)
static int32_t run_one_pass(zp_ctx *ctx, NttPlan *pl, int i, const NttRunOpts &opts, const u64 *cur, u64 cur_cs, u64 in_valid, u64 *nxt, int w) {
    const int logn = pl->logn, m = pl->npass;
    const bool last = (i == m - 1);
    PassArgs a;
    memset(&a, 0, sizeof(a));
    a.in = cur;
    a.out = nxt;
    a.in_cs = cur_cs;
    a.out_cs = 1ULL << logn;
    a.in_valid = in_valid;
    a.twl = pl->d_twl;
    a.twh = pl->d_twh;
    a.lb = pl->lb;
    a.tws = pl->d_tws;
    a.tw1 = (i == 0 && zpi_plan_uses_tw1(ctx, pl)) ? pl->d_tw1 : nullptr;
    a.scale = pl->ninv;
    a.logn = logn;
    a.logPprev = pl->pass[i].logPprev;
    a.j0inv = pl->j0inv;
    // opts.seam_last: the plan's last pass is the seam kernel's built-in one, which takes no input-side table; neither does a last pass
    // that multiplies by coset powers (MODE 2: the inverse side of an extension run as two transforms)
    const bool in_tab = pl->d_itab && zpi_plan_uses_itab(pl) && !opts.seam_last && !opts.post_scale;
    a.flags = last ? 0 : (i == m - 2 && in_tab) ? 8 : 1 | (i >= 1 ? 8 : 0);
    if (last && in_tab) {
        a.itab = pl->d_itab;
        a.logPin = pl->pass[m - 2].logPprev;
    }
    if (last) set_output_scaling(a, pl->inverse && !in_tab, opts.post_scale);
    PassTimer timer(ctx, (i == 0) ? -pl->pass[i].L : pl->pass[i].L);
    return dispatch_pass(ctx, pl->pass[i], a, i == 0, w);
}
// the first pass's full table (8 bytes per element of ONE column, shared by all columns and all later calls of this size):
// built at the first use of a plan by radix-2^7 / 2^8 two-round passes below 2^29 rows; and the last pass's input-side table
static int32_t ensure_tw1(zp_ctx *ctx, NttPlan *pl) {
    const int logn = pl->logn;
    if (!pl->d_tw1 && zpi_plan_uses_tw1(ctx, pl)) {
        if (hipMalloc((void **)&pl->d_tw1, sizeof(u64) << logn) != hipSuccess) {
            // the table is an optimisation (8 bytes per row, per plan, per ctx): without it the first pass multiplies by per-lane
            // twiddle chains (MODE 1), same results.  Clear the sticky error and do not try again for this plan.
            (void)hipGetLastError();
            pl->d_tw1 = nullptr;
            pl->tw1_unavailable = true;
        } else {
            hipLaunchKernelGGL(tw1_fill_kernel, dim3((unsigned)(((1ULL << logn) + 255) / 256)), dim3(256), 0, ctx->stream, pl->d_tw1, logn, pl->pass[0].L,
                               pl->d_twl, pl->d_twh, pl->lb);
            ZP_HIP(ctx, hipGetLastError());
        }
    }
    if (!pl->d_itab && zpi_plan_uses_itab(pl)) {
        const int m = pl->npass, lr = pl->pass[m - 1].L;
        const u64 total = 1ULL << (pl->pass[m - 2].L + lr);
        if (hipMalloc((void **)&pl->d_itab, total * sizeof(u64)) != hipSuccess) {
            // as above: without it the pass before the last multiplies on its output side, same results
            (void)hipGetLastError();
            pl->d_itab = nullptr;
            pl->itab_unavailable = true;
        } else {
            hipLaunchKernelGGL(itab_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, pl->d_itab, total, logn, lr,
                               pl->pass[m - 2].logPprev, pl->inverse ? pl->ninv : 1ULL, pl->d_twl, pl->d_twh, pl->lb);
            ZP_HIP(ctx, hipGetLastError());
        }
    }
    return ZP_OK;
}

int32_t zpi_ntt_run(zp_ctx *ctx, const u64 *d_in, u64 *d_out, int logn, int W, bool inverse,
                    const NttRunOpts &opts) {
    ZP_ARG(ctx, logn >= 0 && logn <= 32, "logn must be in [0,32]");
    ZP_ARG(ctx, W >= 0, "W must be >= 0");
    ZP_ARG(ctx, d_in && d_out, "null device pointer");
    if (W == 0) return ZP_OK;
    NttPlan *pl;
    ZP_TRY(zpi_get_plan(ctx, logn, inverse, &pl));
    const u64 N = 1ULL << logn;
    const u64 in_valid = opts.in_valid_log >= 0 ? (1ULL << opts.in_valid_log) : N;
    ZP_ARG(ctx, in_valid <= N, "in_valid_log > logn");
    ZP_ARG(ctx, !(in_valid != N && (const u64 *)d_out == d_in), "zero-padded input cannot be in place");

    if (logn <= 12) {
        SmallArgs a;
        memset(&a, 0, sizeof(a));
        a.in = d_in;
        a.out = d_out;
        a.in_cs = in_valid;
        a.out_cs = N;
        a.in_valid = in_valid;
        a.tws = pl->d_tws;
        a.scale = pl->ninv;
        a.logn = logn;
        set_output_scaling(a, pl->inverse, opts.post_scale);
        // in place is safe: a block owns its column and loads all of it into LDS before storing
        // in-wave stages where they measured faster (profiles/r5_dpp_ab.txt: <= 64 points 1.1-1.75x; from 2^8 points the doubled arithmetic loses)
        const bool wave = ctx->tune_ntt_small_wave == 1 || (ctx->tune_ntt_small_wave == 0 && logn <= 6);
        hipLaunchKernelGGL(wave ? ntt_small_kernel<true> : ntt_small_kernel<false>, dim3((unsigned)W), dim3(256), (size_t)N * sizeof(u64), ctx->stream, a);
        ZP_HIP(ctx, hipGetLastError());
        return ZP_OK;
    }

    const int wc = chunk_columns(ctx, logn, W);
    const int m = pl->npass;
    ZP_TRY(ensure_tw1(ctx, pl));
    u64 *s0 = nullptr, *s1 = nullptr;
    if (m >= 2) ZP_TRY(zpi_scratch(ctx, 0, (size_t)wc << logn, &s0));
    if (m >= 3) ZP_TRY(zpi_scratch(ctx, 1, (size_t)wc << logn, &s1));

    for (int c0 = 0; c0 < W; c0 += wc) {
        const int w = (W - c0 < wc) ? (W - c0) : wc;
        const u64 *cur = d_in + (u64)c0 * in_valid;
        u64 cur_cs = in_valid;
        for (int i = 0; i < m; i++) {
            const bool last = (i == m - 1);
            u64 *nxt = last ? d_out + ((u64)c0 << logn) : ((i & 1) ? s1 : s0);
            ZP_TRY(run_one_pass(ctx, pl, i, opts, cur, cur_cs, (i == 0) ? in_valid : N, nxt, w));
            cur = nxt;
            cur_cs = N;
        }
    }
    return ZP_OK;
}

// the fused route of zpi_lde (lde_route): inverse passes but the last, the seam kernel, forward passes from the second on; W columns in chunks of wc
static int32_t lde_fused(zp_ctx *ctx, const LdeRoute &r, const CosetTable *ct, const u64 *d_in, u64 *d_out, u64 *d_coef, int logn, int W, int wc) {
    NttPlan *pi = r.inv, *pf = r.fwd;
    const u64 N = 1ULL << logn;
    const int mi = pi->npass, mf = pf->npass;
    const int wf = wc >= 2 ? wc / 2 : 1;                      // columns per forward sub-chunk (2N rows each)
    const size_t need = (size_t)(wc > 2 * wf ? wc : 2 * wf) << logn;
    u64 *s0 = nullptr, *s1 = nullptr, *s2 = nullptr;
    ZP_TRY(zpi_scratch(ctx, 0, need, &s0));
    ZP_TRY(zpi_scratch(ctx, 1, need, &s1));
    if (mf >= 3) ZP_TRY(zpi_scratch(ctx, 2, (size_t)wf << (logn + 1), &s2));
    NttRunOpts none, inv_side;
    inv_side.seam_last = true;
    for (int c0 = 0; c0 < W; c0 += wc) {
        const int w = (W - c0 < wc) ? (W - c0) : wc;
        const u64 *cur = d_in + (u64)c0 * N;
        for (int i = 0; i + 1 < mi; i++) {                     // the inverse transform up to its last pass
            u64 *nxt = (i & 1) ? s1 : s0;
            ZP_TRY(run_one_pass(ctx, pi, i, inv_side, cur, N, N, nxt, w));
            cur = nxt;
        }
        u64 *seam_out = (cur == s0) ? s1 : s0;
        for (int h0 = 0; h0 < w; h0 += wf) {
            const int wh = (w - h0 < wf) ? (w - h0) : wf;
            SeamArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.in = cur + (u64)h0 * N;
            sa.out = seam_out;
            sa.coef = d_coef ? d_coef + (u64)(c0 + h0) * N : nullptr;
            sa.tws_i = pi->d_tws;
            sa.tws_f = pf->d_tws;
            sa.tw1 = pf->d_tw1;
            sa.csl = ct->d_lo;
            sa.csh = ct->d_hi;
            sa.cslb = ct->lb;
            sa.scale = pi->ninv;
            sa.logn = logn;
            sa.j0inv_i = pi->j0inv;
            sa.j0inv_f = pf->j0inv;
            sa.ncols = wh;
            {
                PassTimer timer(ctx, 88);
                hipLaunchKernelGGL(lde_seam_kernel, dim3((unsigned)(((N >> 12) / r.tpw) * (u64)wh)), dim3(256), (size_t)(256 * 16 + 3 * 256) * sizeof(u64), ctx->stream, sa, r.tpw);
                ZP_HIP(ctx, hipGetLastError());
            }
            const u64 *fc = seam_out;                           // the forward transform from its second pass on
            u64 *out = d_out + ((u64)(c0 + h0) << (logn + 1));
            for (int i = 1; i < mf; i++) {
                u64 *nxt = (i == mf - 1) ? out : s2;
                ZP_TRY(run_one_pass(ctx, pf, i, none, fc, 2 * N, 2 * N, nxt, wh));
                fc = nxt;
            }
        }
    }
    return ZP_OK;
}

int32_t zpi_lde(zp_ctx *ctx, const u64 *d_in, u64 *d_out, u64 *d_coef, int logn, int logb, int W, u64 shift) {
    ZP_ARG(ctx, logn >= 0 && logb >= 0 && logn + logb <= 32, "logn/logb out of range");
    ZP_ARG(ctx, W >= 0, "W must be >= 0");
    ZP_ARG(ctx, d_in && d_out, "null device pointer");
    ZP_ARG(ctx, d_out != d_in, "zp_lde cannot run in place");
    if (W == 0) return ZP_OK;
    if (shift == 0) shift = ctx->coset_shift;
    ZP_ARG(ctx, shift < GL_P, "shift not canonical");
    CosetTable *ct;
    ZP_TRY(zpi_get_coset(ctx, logn, shift, 1, &ct));
    const int wc = chunk_columns(ctx, logn, W);
    const LdeRoute r = lde_route(ctx, logn, logb, d_coef != nullptr);
    if (r.fused) {
        ZP_TRY(ensure_tw1(ctx, r.fwd));
        ZP_TRY(ensure_tw1(ctx, r.inv));
        if (r.fwd->d_tw1) return lde_fused(ctx, r, ct, d_in, d_out, d_coef, logn, W, wc);
    }
    // the two-launch route: the inverse transform (its last pass multiplies c_i by shift^i) into the coefficient buffer, the zero-padded forward one out of it
    const u64 N = 1ULL << logn;
    u64 *scaled = nullptr;
    if (!d_coef) ZP_TRY(zpi_scratch(ctx, 2, (size_t)wc << logn, &scaled));
    for (int c0 = 0; c0 < W; c0 += wc) {
        const int w = (W - c0 < wc) ? (W - c0) : wc;
        const u64 *in = d_in + (u64)c0 * N;
        u64 *out = d_out + ((u64)c0 << (logn + logb));
        NttRunOpts inv;
        inv.post_scale = ct;
        // d_coef (optional) IS the scaled-coefficient buffer: the interpolant composed with the coset shift, c_i * shift^i.
        // Nothing downstream needs the plain c_i: p(z) = sum_i (c_i shift^i) (z / shift)^i  (stark/prover.py evaluates there),
        // so the separate copy + scaling pass of round 1 (32*N bytes per column) is gone.
        u64 *sc = d_coef ? d_coef + (u64)c0 * N : scaled;
        ZP_TRY(zpi_ntt_run(ctx, in, sc, logn, w, true, inv));
        NttRunOpts fwd;
        fwd.in_valid_log = logn;  // zero padding is implicit: rows >= N read as 0
        ZP_TRY(zpi_ntt_run(ctx, sc, out, logn + logb, w, false, fwd));
    }
    return ZP_OK;
}

// what zp_lde(blow-up 2) does at this size, as JSON (zp_ntt_plan_json's "lde" member): whether the seam kernel is taken and the radices
// on both sides of it
int32_t zpi_lde_plan_json(zp_ctx *ctx, int logn, int want_coef, std::string *out) {
    LdeRoute r = lde_route(ctx, logn, 1, want_coef != 0);
    if (!r.fused) {
        if (logn + 1 > 32) return ZP_ERR_ARG;
        ZP_TRY(zpi_get_plan(ctx, logn, true, &r.inv));
        ZP_TRY(zpi_get_plan(ctx, logn + 1, false, &r.fwd));
    }
    auto digits = [](const NttPlan *p) {
        std::string d = "[";
        for (int i = 0; i < p->npass; i++) d += (i ? ", " : "") + std::to_string(p->pass[i].L);
        return d + "]";
    };
    *out = std::string("{\"blowup\": 2, \"coefficients_stored\": ") + (want_coef ? "true" : "false") + ", \"seam_fused\": " + (r.fused ? "true" : "false") +
           ", \"inverse_radix_logs\": " + digits(r.inv) + ", \"forward_radix_logs\": " + digits(r.fwd) + "}";
    return ZP_OK;
}

int32_t zpi_twiddle_rows(zp_ctx *ctx, u64 *d_rows, int logn_row, int W, u64 row0, int logn_total, bool inverse) {
    NttPlan *pl;
    ZP_TRY(zpi_get_plan(ctx, logn_total, inverse, &pl));
    const u64 total = (u64)W << logn_row;
    const u64 nmask = logn_total >= 64 ? ~0ULL : ((1ULL << logn_total) - 1);
    hipLaunchKernelGGL(twiddle_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_rows, logn_row,
                       total, row0, nmask, pl->d_twl, pl->d_twh, pl->lb);
    ZP_HIP(ctx, hipGetLastError());
    return ZP_OK;
}
