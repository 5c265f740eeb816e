// The sparse periodic fixed columns of a constraint program at MANY out-of-domain points, on the device: the hot part of
// zp_program_fixed_eval_ext_batch (csrc/verify.hip holds the export, the validation, the two selector columns and the host path).
// A verifier of an aggregated proof needs the fixed columns of one verifier AIR (~10^2 columns, ~4 x 10^5 entries) at the zeta of every header of
// a tree: (point, column, entry) triples, all independent.  Column k with period p = 2^lp at zeta is
//     (y^p - 1) * sum_e c_e / (y - w_e),   y = zeta^(N / p),  w_e = w_p^pos_e,  c_e = value_e w_e / p        (csrc/verify.hip: fixed_col_at)
// What depends on (program, logn, root32) alone -- w_e, c_e (or w_e / p and the public-input index), the cut of the columns into segments -- is
// made once on the host and kept on the ctx; y comes from a table of zeta^(2^k) the host makes per point (<= 32 squarings).
//   fixed_frac_kernel    one workgroup per (point, segment of <= 1024 entries of one column): a lane strides over the entries and keeps the
//                        partial sum as a FRACTION (num, den) in F_{p^3}: num/den + c/d = (num d + c den) / (den d), 21 base-field products per
//                        entry and no inversion; fractions are combined across the wave by shuffles and across the four waves through LDS.
//   fixed_finish_kernel  one lane per (point, column): combines the column's segment fractions, inverts den once and multiplies by y^p - 1 =
//                        zeta^N - 1.  den = 0 is exactly "zeta lies on this column's domain at an entry with a nonzero value": the point is flagged.
// Two launches, no communication between workgroups inside one.  F_{p^3} arithmetic is exact and every value canonical, so the words equal the
// host's bit for bit in whatever order the sum runs (tests/test_fixed_eval_batch.py compares them on both sides of "fixed_eval_dev_min").
// No reference counterpart; the checker's statement of the same sum: oracle/air_program.py fixed_eval_ext.
#include <cstring>
#include <vector>

#include "ctx.hpp"

struct FxSeg { u32 first, count, k, col; };            // entries [first, first + count) of column col; y = zeta^(2^k), k = logn - lp
struct FxCol { u32 seg_first, seg_count; };

struct ZpFixedEvalEntry {
    std::vector<uint64_t> words;                       // the program the tables were made for
    int logn = 0;
    u64 root32 = 0;
    u32 n_cols = 0, n_seg = 0;
    size_t n_entries = 0;
    u64 *d_w = nullptr, *d_c = nullptr;                // per entry
    u32 *d_pub = nullptr;                              // per entry: public-input index, or FX_NOT_PUB
    FxSeg *d_seg = nullptr;
    FxCol *d_col = nullptr;
};
struct ZpFixedEvalCache { std::vector<ZpFixedEvalEntry> entries; };

namespace {

constexpr u32 FX_NOT_PUB = 0xFFFFFFFFu;
constexpr u32 FX_SEG = 1024;                           // entries per workgroup: four per lane
constexpr int FX_BLOCK = 256;

struct frac { e3 n, d; };
__device__ __forceinline__ frac frac_add(const frac &a, const frac &b) {
    return frac{e3_add(e3_mul(a.n, b.d), e3_mul(b.n, a.d)), e3_mul(a.d, b.d)};
}
__device__ __forceinline__ e3 e3_shfl_down(const e3 &a, int delta) {
    return e3_make(__shfl_down(a.c[0], delta), __shfl_down(a.c[1], delta), __shfl_down(a.c[2], delta));
}
__device__ __forceinline__ e3 e3_load(const u64 *p) { return e3_make(p[0], p[1], p[2]); }

// grid (n_seg, points of this launch); partial[(point * n_seg + seg) * 6 ..] = (num, den) of the segment at the point
__global__ void __launch_bounds__(FX_BLOCK) fixed_frac_kernel(const u64 *__restrict__ ew, const u64 *__restrict__ ec, const u32 *__restrict__ epub,
                                                              const FxSeg *__restrict__ segs, u32 n_seg, const u64 *__restrict__ ypow, u32 n_pow,
                                                              const u64 *__restrict__ pubs, u32 n_pubchal, u64 *__restrict__ partial) {
    __shared__ u64 sh[FX_BLOCK / 64][6];
    const u32 s = blockIdx.x, pt = blockIdx.y;
    const FxSeg sg = segs[s];
    const e3 y = e3_load(ypow + ((size_t)pt * n_pow + sg.k) * 3);
    const u64 *pb = pubs + (size_t)pt * n_pubchal;
    frac f{e3_make(0, 0, 0), e3_make(1, 0, 0)};
    for (u32 i = threadIdx.x; i < sg.count; i += FX_BLOCK) {
        const u32 e = sg.first + i;
        u64 c = ec[e];
        const u32 pi = epub[e];
        if (pi != FX_NOT_PUB) c = gl_mul(c, pb[pi]);
        if (c == 0) continue;                          // a zero entry is no term of the sum (and no pole: the host skips it the same way)
        const e3 d = e3_make(gl_sub(y.c[0], ew[e]), y.c[1], y.c[2]);
        f.n = e3_add(e3_mul(f.n, d), e3_scale(f.d, c));
        f.d = e3_mul(f.d, d);
    }
    for (int delta = 32; delta >= 1; delta >>= 1) {
        const frac o{e3_shfl_down(f.n, delta), e3_shfl_down(f.d, delta)};
        f = frac_add(f, o);                            // lanes >= delta compute garbage nobody reads
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int j = 0; j < 3; j++) { sh[wave][j] = f.n.c[j]; sh[wave][3 + j] = f.d.c[j]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FX_BLOCK / 64; w++) f = frac_add(f, frac{e3_load(&sh[w][0]), e3_load(&sh[w][3])});
        u64 *o = partial + ((size_t)pt * n_seg + s) * 6;
        for (int j = 0; j < 3; j++) { o[j] = f.n.c[j]; o[3 + j] = f.d.c[j]; }
    }
}

// one lane per (point, column): out[(point * n_cols + col) * 3 ..] = the column at the point; on_domain[point] = 1 where a denominator vanished
__global__ void __launch_bounds__(FX_BLOCK) fixed_finish_kernel(const FxCol *__restrict__ cols, u32 n_cols, u32 n_seg, u32 n_points, const u64 *__restrict__ partial,
                                                                const u64 *__restrict__ zh, u64 *__restrict__ out, u32 *__restrict__ on_domain) {
    const size_t t = (size_t)blockIdx.x * FX_BLOCK + threadIdx.x;
    if (t >= (size_t)n_points * n_cols) return;
    const u32 pt = (u32)(t / n_cols), col = (u32)(t % n_cols);
    const FxCol fc = cols[col];
    frac f{e3_make(0, 0, 0), e3_make(1, 0, 0)};
    for (u32 s = 0; s < fc.seg_count; s++) {
        const u64 *p = partial + ((size_t)pt * n_seg + fc.seg_first + s) * 6;
        f = frac_add(f, frac{e3_load(p), e3_load(p + 3)});
    }
    u64 det;
    const e3 adj = e3_adj(f.d, &det);
    e3 v = e3_make(0, 0, 0);
    if (det == 0) on_domain[pt] = 1;                   // every writer stores the same word
    else v = e3_mul(e3_mul(f.n, e3_scale(adj, gl_inv(det))), e3_load(zh + (size_t)pt * 3));
    u64 *o = out + t * 3;
    o[0] = v.c[0]; o[1] = v.c[1]; o[2] = v.c[2];
}

void entry_free(ZpFixedEvalEntry &e) {
    if (e.d_w) (void)hipFree(e.d_w);
    if (e.d_c) (void)hipFree(e.d_c);
    if (e.d_pub) (void)hipFree(e.d_pub);
    if (e.d_seg) (void)hipFree(e.d_seg);
    if (e.d_col) (void)hipFree(e.d_col);
    e.d_w = e.d_c = nullptr; e.d_pub = nullptr; e.d_seg = nullptr; e.d_col = nullptr;
}

template <class T>
int32_t upload_vec(zp_ctx *ctx, const std::vector<T> &h, T **d) {
    ZP_HIP(ctx, hipMalloc((void **)d, (h.empty() ? 1 : h.size()) * sizeof(T)));
    if (!h.empty()) ZP_HIP(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return ZP_OK;
}

// the tables of one (program, logn, root32): entries with a constant value of zero are dropped here
int32_t entry_build(zp_ctx *ctx, const uint64_t *prog, size_t program_words, const std::vector<ZpFixedCol> &cols, int logn, u64 root32, ZpFixedEvalEntry *out) {
    std::vector<u64> w, c;
    std::vector<u32> pub;
    std::vector<FxSeg> segs;
    std::vector<FxCol> fcols;
    for (size_t k = 0; k < cols.size(); k++) {
        const ZpFixedCol &fc = cols[k];
        const u64 wp = fc.lp ? gl_root(root32, fc.lp) : 1, pinv = gl_inv((1ULL << fc.lp) % GL_P);
        const int lb = (fc.lp + 1) / 2;                // w_p^pos from a two-level table, as the host path makes it
        std::vector<u64> lo((size_t)1 << lb), hi((size_t)1 << (fc.lp - lb));
        lo[0] = 1;
        for (size_t i = 1; i < lo.size(); i++) lo[i] = gl_mul(lo[i - 1], wp);
        const u64 wl = gl_mul(lo.back(), wp);
        hi[0] = 1;
        for (size_t i = 1; i < hi.size(); i++) hi[i] = gl_mul(hi[i - 1], wl);
        const size_t first = w.size();
        for (size_t e = 0; e < fc.n_entries; e++) {
            const ZpFixedEntry en = zpi_fixed_entry(prog, fc, e);
            const bool is_pub = en.is_pub;
            const u64 v = en.value, pos = en.pos;
            if (!is_pub && v == 0) continue;
            const u64 wj = gl_mul(lo[pos & (((u64)1 << lb) - 1)], hi[pos >> lb]);
            w.push_back(wj);
            c.push_back(is_pub ? gl_mul(wj, pinv) : gl_mul(gl_mul(v, wj), pinv));
            pub.push_back(is_pub ? (u32)v : FX_NOT_PUB);
        }
        if (w.size() >= (1ULL << 31) || segs.size() >= (1u << 30)) return ZP_ERR_UNSUPPORTED;
        FxCol col{(u32)segs.size(), 0};
        for (size_t at = first; at < w.size(); at += FX_SEG) {
            const size_t n = w.size() - at < FX_SEG ? w.size() - at : FX_SEG;
            segs.push_back(FxSeg{(u32)at, (u32)n, (u32)(logn - fc.lp), (u32)k});
            col.seg_count++;
        }
        fcols.push_back(col);
    }
    ZpFixedEvalEntry e;
    e.logn = logn; e.root32 = root32;
    e.n_cols = (u32)cols.size(); e.n_seg = (u32)segs.size(); e.n_entries = w.size();
    int32_t rc = upload_vec(ctx, w, &e.d_w);
    if (rc == ZP_OK) rc = upload_vec(ctx, c, &e.d_c);
    if (rc == ZP_OK) rc = upload_vec(ctx, pub, &e.d_pub);
    if (rc == ZP_OK) rc = upload_vec(ctx, segs, &e.d_seg);
    if (rc == ZP_OK) rc = upload_vec(ctx, fcols, &e.d_col);
    if (rc != ZP_OK) { entry_free(e); return rc; }
    e.words.assign(prog, prog + program_words);
    *out = std::move(e);
    return ZP_OK;
}

}  // namespace

void zpi_fixed_eval_cache_free(zp_ctx *ctx) {
    if (!ctx->fixed_eval_cache) return;
    for (auto &e : ctx->fixed_eval_cache->entries) entry_free(e);
    delete ctx->fixed_eval_cache;
    ctx->fixed_eval_cache = nullptr;
}

// h_sparse u64[n_points][cols.size()][3]: the sparse columns (fixed columns 2..) at every point; h_on_domain[i] = 1 where a denominator of point i
// vanished (its rows of h_sparse are then zero).  The caller (csrc/verify.hip) has validated the blob (`cols` is its table, every lp <= logn), the
// canonical form of every input word and n_pubchal = n_pub + n_chal.
int32_t zpi_fixed_eval_device(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const std::vector<ZpFixedCol> &cols, const uint64_t *h_pubchal,
                              int32_t n_pubchal, int32_t logn, uint64_t root32, const uint64_t *h_zeta, int32_t n_points, uint64_t *h_sparse, uint8_t *h_on_domain) {
    ZpStage stage(ctx, "fixed_eval_batch");
    if (n_points <= 0 || cols.empty()) return ZP_OK;
    try {
        if (!ctx->fixed_eval_cache) ctx->fixed_eval_cache = new ZpFixedEvalCache;
        auto &ents = ctx->fixed_eval_cache->entries;
        ZpFixedEvalEntry *ent = nullptr;
        for (auto &e : ents)
            if (e.logn == logn && e.root32 == root32 && e.words.size() == program_words && memcmp(e.words.data(), h_program, program_words * 8) == 0) ent = &e;
        if (!ent) {
            ZpFixedEvalEntry fresh;
            ZP_TRY(entry_build(ctx, h_program, program_words, cols, logn, root32, &fresh));
            if (ents.size() >= 4) {                    // the oldest goes (nothing of it is in flight: every call ends synchronised)
                entry_free(ents.front());
                ents.erase(ents.begin());
            }
            ents.push_back(std::move(fresh));
            ent = &ents.back();
        }
        const u32 n_cols = ent->n_cols, n_seg = ent->n_seg, n_pow = (u32)logn + 1, npc = (u32)(n_pubchal > 0 ? n_pubchal : 0);
        // per launch at most 2^15 points (grid.y) and 2^24 words (128 MiB) of inputs and fractions
        size_t chunk = ((size_t)1 << 24) / ((size_t)n_seg * 6 + (size_t)n_pow * 3 + 3 + npc);
        chunk = chunk < 1 ? 1 : chunk > ((size_t)1 << 15) ? (size_t)1 << 15 : chunk;
        if (chunk > (size_t)n_points) chunk = (size_t)n_points;
        // one device buffer: [ypow | zh | pubs | partial | out | flags]
        const size_t o_pow = 0, o_zh = o_pow + chunk * n_pow * 3, o_pub = o_zh + chunk * 3, o_part = o_pub + chunk * npc, o_out = o_part + chunk * n_seg * 6,
                     o_flag = o_out + chunk * n_cols * 3, total = o_flag + (chunk + 1) / 2;
        std::vector<u64> h_in(o_part), h_out(chunk * n_cols * 3);
        std::vector<u32> h_flag(chunk);
        u64 *d = nullptr;
        ZP_HIP(ctx, hipMalloc((void **)&d, total * sizeof(u64)));
        int32_t rc = ZP_OK;
        auto hip = [&](hipError_t e, const char *what) {
            if (e != hipSuccess && rc == ZP_OK) { ctx->err = std::string(what) + ": " + hipGetErrorString(e); rc = e == hipErrorOutOfMemory ? ZP_ERR_NOMEM : ZP_ERR_HIP; }
            return rc == ZP_OK;
        };
        for (size_t p0 = 0; p0 < (size_t)n_points && rc == ZP_OK; p0 += chunk) {
            const size_t np = (size_t)n_points - p0 < chunk ? (size_t)n_points - p0 : chunk;
            for (size_t i = 0; i < np; i++) {
                const uint64_t *z = h_zeta + 3 * (p0 + i);
                e3 t = e3_make(z[0], z[1], z[2]);
                for (u32 k = 0; k < n_pow; k++) {
                    memcpy(&h_in[o_pow + (i * n_pow + k) * 3], t.c, 24);
                    if (k + 1 < n_pow) t = e3_mul(t, t);
                }
                const e3 zh = e3_make(gl_sub(t.c[0], 1), t.c[1], t.c[2]);      // t = zeta^N
                memcpy(&h_in[o_zh + i * 3], zh.c, 24);
                if (npc) memcpy(&h_in[o_pub + i * npc], h_pubchal + (p0 + i) * npc, (size_t)npc * 8);
            }
            if (!hip(hipMemcpyAsync(d, h_in.data(), o_part * sizeof(u64), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(fixed_eval inputs)")) break;
            if (!hip(hipMemsetAsync(d + o_flag, 0, ((chunk + 1) / 2) * sizeof(u64), ctx->stream), "hipMemsetAsync(fixed_eval flags)")) break;
            if (n_seg) {
                hipLaunchKernelGGL(fixed_frac_kernel, dim3(n_seg, (unsigned)np), dim3(FX_BLOCK), 0, ctx->stream, ent->d_w, ent->d_c, ent->d_pub, ent->d_seg, n_seg,
                                   d + o_pow, n_pow, d + o_pub, npc, d + o_part);
                if (!hip(hipGetLastError(), "fixed_frac_kernel")) break;
            }
            const size_t nt = np * n_cols;
            hipLaunchKernelGGL(fixed_finish_kernel, dim3((unsigned)((nt + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, ctx->stream, ent->d_col, n_cols, n_seg, (u32)np,
                               d + o_part, d + o_zh, d + o_out, (u32 *)(d + o_flag));
            if (!hip(hipGetLastError(), "fixed_finish_kernel")) break;
            if (!hip(hipMemcpyAsync(h_out.data(), d + o_out, nt * 3 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(fixed_eval values)")) break;
            if (!hip(hipMemcpyAsync(h_flag.data(), d + o_flag, np * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(fixed_eval flags)")) break;
            if (!hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(fixed_eval)")) break;
            for (size_t i = 0; i < np; i++) {
                uint64_t *dst = h_sparse + (p0 + i) * n_cols * 3;
                if (h_flag[i]) { h_on_domain[p0 + i] = 1; memset(dst, 0, (size_t)n_cols * 24); }
                else memcpy(dst, &h_out[i * n_cols * 3], (size_t)n_cols * 24);
            }
        }
        if (rc != ZP_OK) (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d);
        return rc;
    } catch (const std::bad_alloc &) {
        return ZP_ERR_NOMEM;
    }
}
