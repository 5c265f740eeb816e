// The out-of-domain side of a constraint program, on the host: what a VERIFIER does with a statement at the point zeta.
// GenFinalProof (proto/prover/v1/prover.proto:130-148; src/prover/provider.rs:472-503) wraps an aggregated proof the CLIENT hands in: before
// the service spends a final STARK and a Groth16 proof on it, it checks natively what the final STARK's witness does not cover -- the
// aggregation STARK's constraint identity at its out-of-domain point (eigen_zeth_amd/stark/verifier.py; round-4 advisor item: "a
// pairing-valid final proof can be produced over an aggregated proof whose arithmetic is false").  The verifier AIR of an aggregation has
// ~10^2 fixed columns with ~4 x 10^5 sparse entries: their values at zeta are sums over the entries with one F_{p^3} inversion each --
// seconds in Python, milliseconds here (one shared inversion per column by Montgomery's trick, columns spread over threads).
// No reference counterpart (the prover behind the gRPC boundary is external); the checker's own statement of the same: oracle/air_program.py
// (fixed_eval_ext, evaluate_ext) -- the tests compare the two.
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "fr254.hpp"
#include "jsoncur.hpp"
#include "sha256.hpp"
#include "poseidon_default_table.inc"      // ctx = NULL verifies with the library's default tables

// What the verifier takes from other translation units, as WEAK references: this file is also built on its own as plain C++ under the host
// sanitizers (tests/test_verify_fuzz.py, tests/test_r1cs_fuzz.py link it without the rest of the library).  The openings of a text are read by
// csrc/proofparse.hip (absent: only ZP_VERIFY_HEADER_ONLY can be served); the device side is csrc/poseidon.hip (absent: only ctx = NULL) and, for the
// fixed columns at many points, csrc/fixed_eval.hip (absent: the host loop).
extern int32_t zpi_proof_queries_scan(const char *text, size_t len, size_t *q_begin, size_t *q_end, int32_t *n_queries, int32_t *has_stage2, int32_t *n_fri, int32_t *widths,
                                      int32_t *depths, int32_t max_trees, bool bn) __attribute__((weak));
extern int32_t zpi_proof_queries_parse(const char *text, size_t q_begin, size_t q_end, int32_t n_queries, int32_t has_stage2, int32_t n_fri, const int32_t *widths,
                                       const int32_t *depths, uint64_t *index, uint64_t *values, uint64_t *paths, bool bn) __attribute__((weak));
extern int32_t zpi_merkle_verify_openings(zp_ctx *ctx, const ZpOpening *ops, size_t n, const u64 *h_roots, size_t n_roots, uint8_t *ok) __attribute__((weak));
extern int32_t zpi_merkle16_verify_openings_bn254(zp_ctx *ctx, const ZpOpening *ops, size_t n, const u64 *h_roots, size_t n_roots, uint8_t *ok) __attribute__((weak));
extern int32_t zpi_fixed_eval_device(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const std::vector<ZpFixedCol> &cols, const uint64_t *h_pubchal,
                                     int32_t n_pubchal, int32_t logn, uint64_t root32, const uint64_t *h_zeta, int32_t n_points, uint64_t *h_sparse, uint8_t *h_on_domain)
    __attribute__((weak));            // csrc/fixed_eval.hip (absent: zp_program_fixed_eval_ext_batch runs on the host whatever the ctx)
extern int32_t zpi_p254_host_tables(zp_ctx *ctx, std::vector<u32> *rc, std::vector<u32> *mds, int *rp) __attribute__((weak));
// the transcripts of a call on the device (absent: the host sponges whatever the knob says): sponge chains from host buffers, one launch and one
// synchronisation each (csrc/poseidon.hip, csrc/poseidon_bn254.hip), and the commitments of long public-input vectors with the kernels that build
// those trees for the prover
extern int32_t zpi_poseidon_chains_host(zp_ctx *ctx, const u64 *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int nchains, u64 *h_rates) __attribute__((weak));
extern int32_t zpi_poseidon254_chains_host(zp_ctx *ctx, const u64 *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int nchains, u64 *h_rates)
    __attribute__((weak));
extern int32_t zpi_publics_digests(zp_ctx *ctx, const std::vector<const std::vector<u64> *> &pubs, u64 *h_out4) __attribute__((weak));
extern int32_t zpi_publics_digests_bn254(zp_ctx *ctx, const std::vector<const std::vector<u64> *> &pubs, u64 *h_out4) __attribute__((weak));

namespace {

inline e3 e3_base(u64 v) { return e3_make(v, 0, 0); }
inline e3 e3_pow2k(e3 a, int k) { for (int i = 0; i < k; i++) a = e3_mul(a, a); return a; }

// g(y) (y^p - 1) form of one sparse periodic column at zeta: sum_e v_e w_p^pos / (p (y - w_p^pos)) * (y^p - 1), y = zeta^(N / p)
enum { FIXED_OK = 0, FIXED_BAD = 1, FIXED_NOMEM = 2, FIXED_ON_DOMAIN = 3 };
int fixed_col_at(const uint64_t *prog, const ZpFixedCol &fc, const uint64_t *pubs, int logn, u64 root32, const e3 &zeta, const e3 &zh, e3 *out) {
    if (fc.lp > logn) return FIXED_BAD;
    const e3 y = e3_pow2k(zeta, logn - fc.lp);
    const u64 wp = fc.lp ? gl_root(root32, fc.lp) : 1;
    const u64 pinv = gl_inv((1ULL << fc.lp) % GL_P);
    // w_p^pos from a two-level table (2 x 2^(lp/2) entries): one product per entry instead of a 64-step power
    const int lb = (fc.lp + 1) / 2;
    std::vector<u64> lo((size_t)1 << lb), hi((size_t)1 << (fc.lp - lb));
    lo[0] = 1;
    for (size_t i = 1; i < lo.size(); i++) lo[i] = gl_mul(lo[i - 1], wp);
    const u64 wl = gl_mul(lo.back(), wp);
    hi[0] = 1;
    for (size_t i = 1; i < hi.size(); i++) hi[i] = gl_mul(hi[i - 1], wl);
    std::vector<e3> den, pre;
    std::vector<u64> coef;
    den.reserve(fc.n_entries); coef.reserve(fc.n_entries);
    for (size_t e = 0; e < fc.n_entries; e++) {
        const ZpFixedEntry en = zpi_fixed_entry(prog, fc, e);
        const u64 val = en.is_pub ? pubs[en.value] % GL_P : en.value, pos = en.pos;
        if (!val) continue;
        const u64 wj = gl_mul(lo[pos & (((u64)1 << lb) - 1)], hi[pos >> lb]);
        coef.push_back(gl_mul(gl_mul(val, wj), pinv));
        den.push_back(e3_make(gl_sub(y.c[0], wj), y.c[1], y.c[2]));
    }
    e3 run = e3_base(1);
    pre.resize(den.size());
    for (size_t i = 0; i < den.size(); i++) { pre[i] = run; run = e3_mul(run, den[i]); }
    u64 det;
    const e3 adj = e3_adj(run, &det);
    if (!den.empty() && det == 0) return FIXED_ON_DOMAIN;
    e3 inv = den.empty() ? e3_base(1) : e3_scale(adj, gl_inv(det));
    e3 acc = e3_base(0);
    for (size_t i = den.size(); i-- > 0;) {
        const e3 dinv = e3_mul(inv, pre[i]);
        inv = e3_mul(inv, den[i]);
        acc = e3_add(acc, e3_scale(dinv, coef[i]));
    }
    *out = e3_mul(acc, zh);
    return FIXED_OK;
}

// fixed columns 0 / 1 at zeta: the Lagrange basis polynomials of the first and the last row, Z_H(zeta) / (N (zeta - 1)) and Z_H(zeta) w^(N-1) / (N (zeta - w^(N-1)));
// false: zeta is one of the two rows
bool selectors_at(const e3 &zeta, const e3 &zh, u64 wlast, u64 ninv, e3 *first, e3 *last) {
    u64 d0, d1;
    const e3 a0 = e3_adj(e3_make(gl_sub(zeta.c[0], 1), zeta.c[1], zeta.c[2]), &d0), a1 = e3_adj(e3_make(gl_sub(zeta.c[0], wlast), zeta.c[1], zeta.c[2]), &d1);
    if (d0 == 0 || d1 == 0) return false;
    *first = e3_mul(e3_scale(zh, ninv), e3_scale(a0, gl_inv(d0)));
    *last = e3_mul(e3_scale(zh, gl_mul(ninv, wlast)), e3_scale(a1, gl_inv(d1)));
    return true;
}

// zp_program_eval_ext's interpreter: the environment of zpi_program_walk over F_{p^3} at the point zeta
struct ExtEnv {
    typedef e3 value;
    static e3 add(const e3 &a, const e3 &b) { return e3_add(a, b); }
    static e3 sub(const e3 &a, const e3 &b) { return e3_sub(a, b); }
    static e3 mul(const e3 &a, const e3 &b) { return e3_mul(a, b); }
    std::vector<e3> file;
    const uint64_t *ev_z, *ev_zw, *pubchal;
    const u64 *consts;
    const e3 *fixed;
    e3 xml;                                      // zeta - w^(N-1)
    uint64_t *h_out;
    e3 &slot(int i) { return file[i]; }
    e3 load(int kind, int idx) const {
        switch (kind) {
            case ZPK_SLOT: return file[idx];
            case ZPK_COL: return e3_make(ev_z[3 * idx], ev_z[3 * idx + 1], ev_z[3 * idx + 2]);
            case ZPK_NEXT: return e3_make(ev_zw[3 * idx], ev_zw[3 * idx + 1], ev_zw[3 * idx + 2]);
            case ZPK_FIXED: return fixed[idx];
            case ZPK_PUB: return e3_base(pubchal[idx]);
            case ZPK_CONST: return e3_base(consts[idx] % GL_P);      // this reader does not ask for canonical constants
            default: return xml;
        }
    }
    void out(int k, const e3 &v) { memcpy(h_out + 3 * k, v.c, 24); }
};

}  // namespace

extern "C" {

// Values of the K constraints of a program at the out-of-domain point of a proof over a trace of 2^logn rows.
//   h_pubchal u64[n_pubchal]: the public inputs, then the stage-2 challenge components (what the prover's interpreter reads as K_PUB)
//   zeta[3]; h_ev_z / h_ev_zw u64[n_cols][3]: the committed columns' evaluations at zeta / zeta w (n_cols must be the program's W + W2)
//   h_out u64[n_out][3]: constraint k at zeta (n_out must be the program's K) (numerators: the caller combines them with its alpha powers and compares with q(zeta) Z_H(zeta))
// Fixed columns: 0 / 1 the first-row / last-row selectors (Lagrange basis polynomials), then the sparse periodic columns; "x - last" is
// zeta - w^(N-1).  ZP_ERR_ARG: malformed program, non-canonical input, zeta on the trace domain (*zeta_on_domain, when given, tells the last from the
// others: to a verifier it is a property of the proof, not a mistake of its caller).  threads <= 0: one per core, at most 16.
static int32_t program_eval_ext_impl(const uint64_t *h_program, size_t program_words, const uint64_t *h_pubchal, int32_t n_pubchal, int32_t logn, uint64_t root32,
                                     const uint64_t zeta3[3], const uint64_t *h_ev_z, const uint64_t *h_ev_zw, int32_t n_cols, uint64_t *h_out, int32_t n_out,
                                     int32_t threads, uint64_t *h_fixed_out, int32_t n_fixed_out, bool *zeta_on_domain = nullptr, const uint64_t *fixed_in = nullptr) {
    if (zeta_on_domain) *zeta_on_domain = false;
    const bool only_fixed = h_fixed_out != nullptr;
    try {
        if (!zeta3 || logn < 1 || logn > 32 || n_pubchal < 0 || (n_pubchal && !h_pubchal)) return ZP_ERR_ARG;
        if (!only_fixed && (!h_ev_z || !h_ev_zw || !h_out)) return ZP_ERR_ARG;
        ZpProgram pg;
        if (!zpi_program_read(h_program, program_words, ZPG_FIXED_EVAL, &pg, nullptr)) return ZP_ERR_ARG;
        const size_t W = pg.W, W2 = pg.W2, n_fixed = pg.n_fixed, K = pg.K;
        const std::vector<ZpFixedCol> &fxc = pg.fxc;
        if ((size_t)n_pubchal != pg.n_pub + pg.n_chal || root32 == 0 || root32 >= GL_P) return ZP_ERR_ARG;
        // the caller's arrays are sized by ITS idea of the statement: they must be the program's (a blob with another width or constraint count
        // would be read / written past them)
        if (!only_fixed && (n_cols < 0 || (size_t)n_cols != W + W2 || n_out < 0 || (size_t)n_out != K)) return ZP_ERR_ARG;
        if (only_fixed && (n_fixed_out < 0 || (size_t)n_fixed_out != n_fixed)) return ZP_ERR_ARG;
        for (int i = 0; i < 3; i++)
            if (zeta3[i] >= GL_P) return ZP_ERR_ARG;
        for (int i = 0; i < n_pubchal; i++)
            if (h_pubchal[i] >= GL_P) return ZP_ERR_ARG;
        const size_t Wt = W + W2;
        for (size_t i = 0; !only_fixed && i < Wt * 3; i++)
            if (h_ev_z[i] >= GL_P || h_ev_zw[i] >= GL_P) return ZP_ERR_ARG;
        const e3 zeta = e3_make(zeta3[0], zeta3[1], zeta3[2]);
        const u64 N = 1ULL << logn, wN = gl_root(root32, logn), wlast = gl_pow(wN, N - 1), ninv = gl_inv(N % GL_P);
        const e3 zN = e3_pow2k(zeta, logn), zh = e3_make(gl_sub(zN.c[0], 1), zN.c[1], zN.c[2]);
        std::vector<e3> fixed(n_fixed);
        if (fixed_in) {                        // u64[n_fixed][3] made by zp_program_fixed_eval_ext_batch for this very (program, public inputs, zeta)
            for (size_t k = 0; k < n_fixed; k++) fixed[k] = e3_make(fixed_in[3 * k], fixed_in[3 * k + 1], fixed_in[3 * k + 2]);
        } else {
            if (!selectors_at(zeta, zh, wlast, ninv, &fixed[0], &fixed[1])) { if (zeta_on_domain) *zeta_on_domain = true; return ZP_ERR_ARG; }
            // the sparse columns over threads (columns differ a lot in length: hand them out one at a time)
            const unsigned nt = fxc.size() < 8 ? 1 : zpi_host_threads(threads);
            std::vector<int> bad(nt, 0);
            zpi_over_threads(nt, [&](unsigned t) noexcept {
                try {
                    for (size_t k = t; k < fxc.size(); k += nt)
                        if (const int r = fixed_col_at(h_program, fxc[k], h_pubchal, logn, root32, zeta, zh, &fixed[2 + k])) { bad[t] = r; return; }
                } catch (...) { bad[t] = FIXED_NOMEM; }
            });
            for (int b : bad)
                if (b == FIXED_NOMEM) return ZP_ERR_NOMEM;
            for (int b : bad)
                if (b == FIXED_BAD) return ZP_ERR_ARG;
            for (int b : bad)
                if (b) { if (zeta_on_domain) *zeta_on_domain = true; return ZP_ERR_ARG; }
        }
        if (only_fixed) {
            for (size_t k = 0; k < n_fixed; k++) memcpy(h_fixed_out + 3 * k, fixed[k].c, 24);
            return ZP_OK;
        }
        // the three-address code in F_{p^3}: the code group first (here, behind the fixed columns: a point on the trace domain is reported as that
        // whatever the code holds), so the walk checks nothing
        if (!zpi_program_check(&pg, ZPG_CODE, nullptr)) return ZP_ERR_ARG;
        ExtEnv env;
        env.file.assign(pg.slot_file(), e3_base(0));
        env.ev_z = h_ev_z; env.ev_zw = h_ev_zw; env.pubchal = h_pubchal; env.consts = pg.consts; env.fixed = fixed.data(); env.h_out = h_out;
        env.xml = e3_make(gl_sub(zeta.c[0], wlast), zeta.c[1], zeta.c[2]);
        zpi_program_walk(pg.ins, (int)pg.n_instr, env);
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

int32_t zp_program_eval_ext(const uint64_t *h_program, size_t program_words, const uint64_t *h_pubchal, int32_t n_pubchal, int32_t logn, uint64_t root32,
                            const uint64_t zeta3[3], const uint64_t *h_ev_z, const uint64_t *h_ev_zw, int32_t n_cols, uint64_t *h_out, int32_t n_out,
                            int32_t threads) {
    return program_eval_ext_impl(h_program, program_words, h_pubchal, n_pubchal, logn, root32, zeta3, h_ev_z, h_ev_zw, n_cols, h_out, n_out, threads, nullptr, 0);
}

// The FIXED columns of a program at the out-of-domain point: h_fixed u64[n_fixed][3] (n_fixed must be the program's): columns 0 / 1 the first-row /
// last-row selectors, then the sparse periodic columns (public-input entries read from h_pubchal).  A function of (statement, public inputs, zeta)
// alone -- what the Groth16 wrap's circuit takes as committed input instead of evaluating ~10^5 entries in F_r (service/wrap_arith.py), and what a
// reader of its public input recomputes.  Same refusals as zp_program_eval_ext.
int32_t zp_program_fixed_eval_ext(const uint64_t *h_program, size_t program_words, const uint64_t *h_pubchal, int32_t n_pubchal, int32_t logn, uint64_t root32,
                                  const uint64_t zeta3[3], uint64_t *h_fixed, int32_t n_fixed, int32_t threads) {
    if (!h_fixed) return ZP_ERR_ARG;
    return program_eval_ext_impl(h_program, program_words, h_pubchal, n_pubchal, logn, root32, zeta3, nullptr, nullptr, 0, nullptr, 0, threads, h_fixed, n_fixed);
}

// The same at n_points points, each with its own public inputs: h_pubchal u64[n_points][n_pubchal], h_zeta u64[n_points][3], h_fixed u64[n_points][n_fixed][3].
// Point by point the results and refusals of zp_program_fixed_eval_ext, but for a zeta on the trace domain or on the domain of one column: that sets
// h_on_domain[i], leaves the point's rows zero and fails nothing (to a verifier a property of one proof).  ctx = NULL, or fewer (points x sparse
// entries) than the knob "fixed_eval_dev_min": the host code above in a loop.  Otherwise the sparse columns of all points in one pass of
// csrc/fixed_eval.hip (the two selectors stay here); F_{p^3} arithmetic is exact, so the two paths give the same words.
int32_t zp_program_fixed_eval_ext_batch(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *h_pubchal, int32_t n_pubchal, int32_t logn,
                                        uint64_t root32, const uint64_t *h_zeta, int32_t n_points, uint64_t *h_fixed, int32_t n_fixed, uint8_t *h_on_domain, int32_t threads) {
    try {
        if (n_points < 0 || (n_points && (!h_zeta || !h_fixed || !h_on_domain)) || logn < 1 || logn > 32 || n_pubchal < 0 || (n_pubchal && n_points && !h_pubchal))
            return ZP_ERR_ARG;
        // the refusals of program_eval_ext_impl that do not depend on the point, once (n_points = 0 is refused like any other count)
        ZpProgram pg;
        if (!zpi_program_read(h_program, program_words, ZPG_FIXED_EVAL, &pg, nullptr)) return ZP_ERR_ARG;
        const std::vector<ZpFixedCol> &fxc = pg.fxc;
        if ((size_t)n_pubchal != pg.n_pub + pg.n_chal || root32 == 0 || root32 >= GL_P || n_fixed < 0 || (size_t)n_fixed != pg.n_fixed) return ZP_ERR_ARG;
        size_t entries = 0;
        for (const ZpFixedCol &fc : fxc) {
            if (fc.lp > logn) return ZP_ERR_ARG;
            entries += fc.n_entries;
        }
        const size_t np = (size_t)n_points, row = (size_t)n_fixed * 3;
        for (size_t i = 0; i < np * 3; i++)
            if (h_zeta[i] >= GL_P) return ZP_ERR_ARG;
        for (size_t i = 0; i < np * (size_t)n_pubchal; i++)
            if (h_pubchal[i] >= GL_P) return ZP_ERR_ARG;
        if (np) { memset(h_on_domain, 0, np); memset(h_fixed, 0, np * row * 8); }
        const bool on_device = ctx && zpi_fixed_eval_device && !fxc.empty() && np && entries &&
                               (ctx->tune_fixed_eval_dev_min <= 0 || np >= ((size_t)ctx->tune_fixed_eval_dev_min + entries - 1) / entries);
        if (!on_device) {
            for (size_t i = 0; i < np; i++) {
                bool on_domain = false;
                const int32_t rc = program_eval_ext_impl(h_program, program_words, n_pubchal ? h_pubchal + i * (size_t)n_pubchal : nullptr, n_pubchal, logn, root32, h_zeta + 3 * i,
                                                         nullptr, nullptr, 0, nullptr, 0, threads, h_fixed + i * row, n_fixed, &on_domain);
                if (rc != ZP_OK && !on_domain) return rc;
                if (rc != ZP_OK) { h_on_domain[i] = 1; memset(h_fixed + i * row, 0, row * 8); }
            }
            return ZP_OK;
        }
        std::vector<u64> sparse(np * fxc.size() * 3);
        ZP_TRY(zpi_fixed_eval_device(ctx, h_program, program_words, fxc, h_pubchal, n_pubchal, logn, root32, h_zeta, n_points, (uint64_t *)sparse.data(), h_on_domain));
        const u64 N = 1ULL << logn, wlast = gl_pow(gl_root(root32, logn), N - 1), ninv = gl_inv(N % GL_P);
        for (size_t i = 0; i < np; i++) {
            const e3 zeta = e3_make(h_zeta[3 * i], h_zeta[3 * i + 1], h_zeta[3 * i + 2]);
            const e3 zN = e3_pow2k(zeta, logn), zh = e3_make(gl_sub(zN.c[0], 1), zN.c[1], zN.c[2]);
            e3 sel[2];
            if (!selectors_at(zeta, zh, wlast, ninv, &sel[0], &sel[1])) h_on_domain[i] = 1;
            if (h_on_domain[i]) continue;              // the point's rows stay zero
            memcpy(h_fixed + i * row, sel[0].c, 24);
            memcpy(h_fixed + i * row + 3, sel[1].c, 24);
            memcpy(h_fixed + i * row + 6, &sparse[i * fxc.size() * 3], fxc.size() * 24);
        }
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

}  // extern "C"

// ================================================================================================================================
// The STARK verifier behind zp_stark_verify / zp_stark_verify_batch (Goldilocks-hash mode) and zp_stark_verify_bn128 / zp_stark_verify_batch_bn128
// (BN128-hash mode: the final STARK of GenFinalProof): what a host that was handed a proof as TEXT asks before it spends anything on it.
// The hash mode is a PARAMETER of the one header phase and the one query phase below.  What BN128 mode changes: roots and path words are quoted
// field elements of F_r (a root >= r is MALFORMED, a path word >= r equals nothing), the transcript is the width-17 sponge (HostSponge254), a long
// public-input vector is committed by the 16-ary tree over rows of 48, a committed leaf holds 2^g rows, and an opening carries the whole group of
// every level (HostPoseidon254::opening_ok; on a ctx csrc/poseidon_bn254.hip: zpi_merkle16_verify_openings_bn254).  No grinding in that mode.  The protocol is stark/prover.py's; the checks and their order are restated here from the
// protocol (the CPU checker's independent statement of the same is oracle/stark_verify.py -- the tests run the two side by side).
// Everything in this file is host code: the header of the text, the transcript (a textbook-schedule Poseidon, the only host one in the
// product), the identity at zeta, the final layer's degree, the DEEP sum and every fold at every query.  The one O(openings) part -- the
// leaf hash and the path of every opening -- goes to the device in one launch when a ctx is given (csrc/poseidon.hip:
// zpi_merkle_verify_openings) and runs here otherwise (ctx = NULL: the sanitizer build and a machine without a GPU).
// Numbers: a number of the text that the protocol takes as a field element (public input, evaluation, opened value, path word) is read
// mod p, as the checker reads it; where the protocol COMPARES a number of the text (parameters, roots, indices, the nonce, an opened FRI
// value against the previous fold) a value >= p equals nothing.
namespace {

using zpjson::Cur;
using zpjson::each_member;

struct HostPoseidon {
    const u64 *rc, *mds;
    void perm(u64 *s) const {                     // ARK -> S-box -> MDS, 4 + 22 + 4 rounds; canonical in and out
        for (int r = 0; r < 30; r++) {
            const bool full = r < 4 || r >= 26;
            for (int i = 0; i < 12; i++) {
                u64 x = gl_add(s[i], rc[r * 12 + i]);
                if (full || i == 0) { const u64 x2 = gl_mul(x, x), x3 = gl_mul(x2, x); x = gl_mul(gl_mul(x2, x2), x3); }
                s[i] = x;
            }
            u64 o[12];
            for (int i = 0; i < 12; i++) {
                unsigned __int128 acc = 0;        // 12 terms < 2^28 * 2^64
                for (int j = 0; j < 12; j++) acc += (unsigned __int128)mds[i * 12 + j] * s[j];
                o[i] = gl_reduce96((u64)acc, (u32)(acc >> 64), 0u);
            }
            memcpy(s, o, sizeof o);
        }
    }
    void pair(const u64 *l, const u64 *r, u64 *out4) const {
        u64 s[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
        perm(s);
        memcpy(out4, s, 32);
    }
    // the leaf hash of zp_merkle_commit: blocks of 8 with the digest so far as the next capacity; <= 4 values are their own digest
    void leaf(const u64 *v, size_t w, u64 *out4) const {
        u64 s[12] = {0};
        if (w <= 4) { for (size_t j = 0; j < 4; j++) out4[j] = j < w ? v[j] : 0; return; }
        for (size_t off = 0; off < w; off += 8) {
            for (size_t j = 0; j < 8; j++) s[j] = off + j < w ? v[off + j] : 0;
            perm(s);
            memcpy(s + 8, s, 32);
        }
        memcpy(out4, s + 8, 32);
    }
    bool opening_ok(const ZpOpening &op, const u64 *root4) const {
        u64 cur[4];
        leaf(op.values, op.width, cur);
        for (uint32_t l = 0; l < op.depth; l++) {
            if ((op.index >> l) & 1) pair(op.path + 4 * l, cur, cur);
            else pair(cur, op.path + 4 * l, cur);
        }
        return memcmp(cur, root4, 32) == 0;
    }
};

// stark/transcript.py: absorb queues; a squeeze first absorbs the queue in blocks that overwrite the rate (one bare permutation when nothing is
// queued), then hands out the rate
struct Transcript {                            // what the header phase asks of either mode's sponge
    virtual void absorb(const u64 *v, size_t n) = 0;
    virtual void absorb_root(const u64 *root4) = 0;      // Goldilocks mode: four elements; BN128 mode: one element of F_r in four words, < r
    virtual void squeeze(size_t n, u64 *out) = 0;
    virtual ~Transcript() {}
    e3 challenge() { u64 c[3]; squeeze(3, c); return e3_make(c[0], c[1], c[2]); }
};

// What a hash mode makes of the queue: BW words per block, NOUT values per rate.
// Goldilocks mode: a value is a word, a root four of them, blocks of 8, the rate as it stands.
struct GlMode {
    static constexpr size_t BW = 8, NOUT = 8;
    static void queue(std::vector<u64> &q, const u64 *v, size_t n) { for (size_t i = 0; i < n; i++) q.push_back(gl_canon(v[i])); }
    static void queue_root(std::vector<u64> &q, const u64 *root4) { queue(q, root4, 4); }
    static void read(const u64 *rate, u64 *avail) { memcpy(avail, rate, 8 * NOUT); }
};
// BN128 mode (oracle/stark_verify.py SpongeBN128; stark/transcript.py TranscriptBN128): an element is four words, standard form; Goldilocks values go
// three to an element (each absorb padded separately), a root is one element; blocks of 16 elements; the rate is read as the three low 64-bit words of
// each of its 16 elements mod p
struct BnMode {
    static constexpr size_t BW = 64, NOUT = 48;
    static void queue(std::vector<u64> &q, const u64 *v, size_t n) {
        for (size_t i = 0; i < n; i += 3) {
            for (size_t c = 0; c < 3; c++) q.push_back(i + c < n ? gl_canon(v[i + c]) : 0);
            q.push_back(0);
        }
    }
    static void queue_root(std::vector<u64> &q, const u64 *root4) { q.insert(q.end(), root4, root4 + 4); }
    static void read(const u64 *rate, u64 *avail) {
        for (int e = 0; e < 16; e++)
            for (int c = 0; c < 3; c++) avail[3 * e + c] = gl_canon(rate[4 * e + c]);
    }
};

// THE block rule, once for both modes and for everything that walks a transcript: a squeeze that finds values queued (or the rate used up) turns the
// queue into STEPS -- (absorb flag, block): one bare permutation when nothing is queued, else one absorbing step per block of BW words, the last
// one zero padded -- and then reads the rate after the last step.  What a step does is the user's: hash (HostSponge, HostSponge254), record
// (PlanSponge), or advance through recorded steps whose rates the device wrote (ReplaySponge).
template <class M>
struct BlockSponge : Transcript {
    std::vector<u64> q;
    u64 avail[M::NOUT];
    size_t pos = M::NOUT;
    virtual void step(bool absorb, const u64 *block) = 0;      // block: BW words (absorb) or NULL
    virtual void rate(u64 *out) = 0;                           // the rate after the last step, BW standard words
    void absorb(const u64 *v, size_t n) override { M::queue(q, v, n); pos = M::NOUT; }
    void absorb_root(const u64 *root4) override { M::queue_root(q, root4); pos = M::NOUT; }
    void squeeze(size_t n, u64 *out) override {
        for (size_t k = 0; k < n; k++) {
            if (!q.empty() || pos == M::NOUT) {
                if (q.empty()) step(false, nullptr);
                for (size_t off = 0; off < q.size(); off += M::BW) {
                    u64 blk[M::BW];
                    for (size_t j = 0; j < M::BW; j++) blk[j] = off + j < q.size() ? q[off + j] : 0;
                    step(true, blk);
                }
                q.clear();
                u64 r[M::BW];
                rate(r);
                M::read(r, avail);
                pos = 0;
            }
            out[k] = avail[pos++];
        }
    }
};

struct HostSponge : BlockSponge<GlMode> {
    const HostPoseidon &H;
    u64 st[12] = {0};
    explicit HostSponge(const HostPoseidon &h) : H(h) {}
    void step(bool absorb, const u64 *block) override { if (absorb) memcpy(st, block, 64); H.perm(st); }
    void rate(u64 *out) override { memcpy(out, st, 64); }
};

// The transcripts of a call as sponge chains (csrc/poseidon.hip: sponge_chains_kernel; csrc/poseidon_bn254.hip: sponge_chains254_kernel): nothing a
// verifier absorbs depends on a challenge, so the steps of every text are known once it is parsed.  Chain c is the steps [first[c], first[c + 1]);
// blocks: bw words per step (zero for a bare step); rates: bw words per step, written by the device.
struct ChainPlan {
    std::vector<u64> blocks, rates;
    std::vector<uint8_t> absorb;
    std::vector<uint32_t> first = {0};
};
// records the steps and returns nothing (every squeezed value reads 0: the schedule of a transcript does not depend on them)
template <class M>
struct PlanSponge : BlockSponge<M> {
    ChainPlan &cp;
    explicit PlanSponge(ChainPlan &c) : cp(c) {}
    void step(bool absorb, const u64 *block) override {
        cp.absorb.push_back(absorb ? 1 : 0);
        if (absorb) cp.blocks.insert(cp.blocks.end(), block, block + M::BW);
        else cp.blocks.resize(cp.blocks.size() + M::BW, 0);
    }
    void rate(u64 *out) override { memset(out, 0, 8 * M::BW); }
    size_t next_word() const { return cp.blocks.size() + this->q.size(); }      // where, in cp.blocks, the next queued word will stand
    void close() { cp.first.push_back((uint32_t)cp.absorb.size()); }
};
// holds a chain's recorded steps and the rates the device wrote: absorbing advances through the plan, squeezing hands out the recorded rate of the
// step it has reached.  A replay that leaves its plan (another step than the recorded one, or one too many) is a bug of this file, never a verdict
struct ReplayLeftPlan {};
template <class M>
struct ReplaySponge : BlockSponge<M> {
    const ChainPlan &cp;
    size_t at, begin, end;
    ReplaySponge(const ChainPlan &c, size_t chain) : cp(c), at(c.first[chain]), begin(c.first[chain]), end(c.first[chain + 1]) {}
    void step(bool absorb, const u64 *block) override {
        if (at >= end || (cp.absorb[at] != 0) != absorb || (absorb && memcmp(&cp.blocks[at * M::BW], block, 8 * M::BW) != 0)) throw ReplayLeftPlan{};
        at++;
    }
    void rate(u64 *out) override {
        if (at == begin) throw ReplayLeftPlan{};
        memcpy(out, &cp.rates[(at - 1) * M::BW], 8 * M::BW);
    }
};

// The sponge above with NO hashing (restated from the protocol of stark/verifier_air.py; the checker's: oracle/stark_verify.py PublicSponge): a
// verifier-AIR STARK vouches for every permutation of an inner proof's transcript, and its public inputs list, in protocol order, the values each
// permutation absorbs (a last block is NOT padded) and the rate after every permutation the protocol reads.  Absorbing compares, squeezing reads;
// anything else than the stream dictates is a TranscriptMismatch.  One stream serves all inner proofs of a node: reset() between them.
struct TranscriptMismatch {};
struct PublicSponge : Transcript {
    const u64 *s;
    size_t n, pos = 0;
    std::vector<u64> q;
    u64 avail[8];
    int apos = 8;
    PublicSponge(const u64 *stream, size_t len) : s(stream), n(len) {}
    const u64 *take(size_t k) { if (k > n - pos) throw TranscriptMismatch{}; pos += k; return s + pos - k; }
    void reset() { q.clear(); apos = 8; }
    void absorb(const u64 *v, size_t k) override { for (size_t i = 0; i < k; i++) q.push_back(gl_canon(v[i])); apos = 8; }
    void absorb_root(const u64 *root4) override { absorb(root4, 4); }
    void squeeze(size_t k, u64 *out) override {
        for (size_t i = 0; i < k; i++) {
            if (!q.empty() || apos == 8) {
                for (size_t off = 0; off < q.size(); off += 8) {
                    const size_t len = q.size() - off < 8 ? q.size() - off : 8;
                    if (memcmp(take(len), &q[off], 8 * len) != 0) throw TranscriptMismatch{};
                }
                q.clear();
                memcpy(avail, take(8), 64);
                for (u64 v : avail) if (v >= GL_P) throw TranscriptMismatch{};      // a rate is a permutation's output: canonical
                apos = 0;
            }
            out[i] = avail[apos++];
        }
    }
    // the grinding hash, the last permutation of a proof's public transcript: seed || nonce in, the rate out
    u64 pow_digest0(const u64 *seed4, u64 nonce) {
        const u64 *in = take(5);
        if (memcmp(in, seed4, 32) != 0 || in[4] != nonce) throw TranscriptMismatch{};
        return take(8)[0];
    }
};

// ---- BN128-hash mode on the host: the product's only host Poseidon-BN254 (t = 17), a textbook-schedule permutation over csrc/fr254.hpp (the device
// kernels walk the sparse form of the same map: csrc/poseidon_bn254.hip); tables in Montgomery limbs, as zp_set_poseidon_bn254 keeps them
inline int levels16(u64 n) { int l = 0; for (; n > 1; n = (n + 15) / 16) l++; return l; }
struct HostPoseidon254 {
    int rp = 0;
    std::vector<u32> rc, mds;                  // [(8 + rp) * 17][9], [17 * 17][9]
    static fr limbs(const u32 *p) { fr x; memcpy(x.l, p, 36); return x; }
    void perm(fr *s) const {                   // ARK -> S-box -> matrix (a row: 6 + 6 + 5 products, one reduction each), 4 + rp + 4 rounds
        for (int r = 0; r < 8 + rp; r++) {
            const bool full = r < 4 || r >= 4 + rp;
            for (int i = 0; i < 17; i++) {
                fr x = fr_add(s[i], limbs(&rc[((size_t)r * 17 + i) * 9]));
                if (full || i == 0) { const fr x2 = fr_sqr(x), x4 = fr_sqr(x2); x = fr_mul(x4, x); }
                s[i] = x;
            }
            fr o[17];
            for (int i = 0; i < 17; i++) {
                const u32 *row = &mds[(size_t)i * 17 * 9];
                o[i] = fr_add(fr_add(fr_dotc<6>(s, row), fr_dotc<6>(s + 6, row + 6 * 9)), fr_dotc<5>(s + 12, row + 12 * 9));
            }
            memcpy(s, o, sizeof o);
        }
    }
    // the digest of [0 | 16 elements of four standard words each, < r]
    void node(const u64 *grp64, u64 *out4) const {
        fr s[17];
        s[0] = fr_zero();
        for (int k = 0; k < 16; k++) s[1 + k] = fr_to_mont(fr_from_u64(grp64 + 4 * k));
        perm(s);
        fr_to_u64(fr_from_mont(s[0]), out4);
    }
    // the leaf hash of zp_merkle16_commit_bn254: a sponge over blocks of 56 values (leaf_block_element), the digest so far as the next capacity
    void leaf(const u64 *v, size_t w, u64 *out4) const {
        fr s[17];
        s[0] = fr_zero();
        for (size_t base = 0; base < w || base == 0; base += 56) {
            for (int k = 0; k < 16; k++) {
                u64 x[4];
                leaf_block_element(v, 1, 0, (int)w, (int)base, k, x);
                s[1 + k] = fr_to_mont(fr_from_u64(x));
            }
            perm(s);
        }
        fr_to_u64(fr_from_mont(s[0]), out4);
    }
    // per level: every word of the group < r, the digest so far at the group's slot pos % 16, children beyond the level's size zero, the next digest
    // the permutation of [0, group]; after the last level the digest is the root.  (width, depth = level count and index were validated by the caller)
    bool opening_ok(const ZpOpening &op, const u64 *root4) const {
        u64 cur[4];
        leaf(op.values, op.width, cur);
        u64 n = op.leaves, pos = op.index;
        for (uint32_t l = 0; l < op.depth; l++, n = (n + 15) / 16, pos /= 16) {
            const u64 *grp = op.path + 64 * (size_t)l, g0 = (pos / 16) * 16;
            for (int c = 0; c < 16; c++) {
                if (!fr_is_canonical_u64(grp + 4 * c)) return false;
                if (g0 + c >= n && (grp[4 * c] | grp[4 * c + 1] | grp[4 * c + 2] | grp[4 * c + 3])) return false;
            }
            if (memcmp(grp + 4 * (pos % 16), cur, 32) != 0) return false;
            node(grp, cur);
        }
        return memcmp(cur, root4, 32) == 0;
    }
};

// the width-17 sponge of BN128 mode on the host: element 0 = capacity, 1..16 = rate (BnMode and the block rule above)
struct HostSponge254 : BlockSponge<BnMode> {
    const HostPoseidon254 &H;
    fr st[17];
    explicit HostSponge254(const HostPoseidon254 &h) : H(h) { for (fr &x : st) x = fr_zero(); }
    void step(bool absorb, const u64 *block) override {
        if (absorb) for (size_t j = 0; j < 16; j++) st[1 + j] = fr_to_mont(fr_from_u64(block + 4 * j));
        H.perm(st);
    }
    void rate(u64 *out) override { for (int e = 0; e < 16; e++) fr_to_u64(fr_from_mont(st[1 + e]), out + 4 * e); }
};

// the same commitment in BN128 mode (publics_rows: rows of 48 values, three to an element, >= 1 row; the 16-ary tree of zp_merkle16_commit_bn254)
void publics_digest_host254(const HostPoseidon254 &H, const std::vector<u64> &pubs, u64 *out4) {
    size_t n = (pubs.size() + 47) / 48;
    n = n ? n : 1;
    std::vector<u64> lvl(4 * n), row(48);
    for (size_t r = 0; r < n; r++) {
        for (size_t j = 0; j < 48; j++) row[j] = 48 * r + j < pubs.size() ? pubs[48 * r + j] : 0;
        H.leaf(row.data(), 48, &lvl[4 * r]);
    }
    for (; n > 1; n = (n + 15) / 16)
        for (size_t r = 0; r < (n + 15) / 16; r++) {
            u64 grp[64] = {0};
            memcpy(grp, &lvl[64 * r], 32 * (16 * r + 16 <= n ? 16 : n - 16 * r));
            H.node(grp, &lvl[4 * r]);
        }
    memcpy(out4, lvl.data(), 32);
}

// the commitment a long public-input vector enters the transcript as (stark/prover.py publics_rows: rows of 8, zero padded, 2^k >= 2 rows)
void publics_digest_host(const HostPoseidon &H, const std::vector<u64> &pubs, u64 *out4) {
    size_t M = 2;
    while (M * 8 < pubs.size()) M <<= 1;
    std::vector<u64> lvl(4 * M);
    for (size_t r = 0; r < M; r++) {
        u64 s[12] = {0};
        for (size_t j = 0; j < 8; j++) s[j] = 8 * r + j < pubs.size() ? pubs[8 * r + j] : 0;
        H.perm(s);
        memcpy(&lvl[4 * r], s, 32);
    }
    for (; M > 1; M >>= 1)
        for (size_t r = 0; r < M / 2; r++) H.pair(&lvl[8 * r], &lvl[8 * r + 4], &lvl[4 * r]);
    memcpy(out4, lvl.data(), 32);
}

// ---- the header of a proof text (everything but "queries")
struct ProofHeader {
    static constexpr int NPARAM = 6;
    bool has_params = false, has_param[NPARAM] = {}, has_root32 = false, has_shift = false, has_digest = false, has_pubs = false, has_nonce = false, has_queries = false;
    bool has_root[3] = {};                     // trace, stage2, quotient
    bool has_z = false, has_zw = false, has_fri_roots = false, has_final = false;
    uint64_t param[NPARAM] = {}, root32 = 0, shift = 0, nonce = 0;
    std::string hash = "gl", digest;
    std::vector<u64> pubs, root[3], ev_z, ev_zw, fri_roots;
    std::vector<std::vector<u64>> final_l;
    bool rows_ok = true;                       // every row of the evaluations has 3 words, every root 4 (BN128 mode: one quoted element, kept as its 4 words)
};
const char *const PARAM_KEYS[ProofHeader::NPARAM] = {"logn", "logb", "fri_logf", "fri_final_log", "n_queries", "pow_bits"};

bool once(Cur &c, bool &got) { if (got) c.ok = false; got = true; return c.ok; }      // a repeated key is not this grammar

bool u64_list(Cur &c, std::vector<u64> *out) {
    if (!c.need('[')) return false;
    if (c.eat(']')) return true;
    for (;;) {
        uint64_t v;
        if (!c.u64v(&v)) return c.ok = false;
        out->push_back(v);
        if (c.eat(',')) continue;
        return c.need(']');
    }
}
// BN128 mode: a root, ["<decimal>"] -- one quoted element, kept as four words (anything else in the list clears *rows_ok; a plain number is read so
// that a Goldilocks-mode text reaches the check of its hash mode)
bool fr_root(Cur &c, std::vector<u64> *out, bool *rows_ok) {
    if (!c.need('[')) return false;
    size_t count = 0;
    if (!c.eat(']'))
        for (;;) {
            uint64_t w[4] = {0, 0, 0, 0};
            if (c.peek('"')) { if (!c.dec256(w)) return false; }
            else { if (!c.u64v(w)) return c.ok = false; *rows_ok = false; }
            if (count++ == 0) out->insert(out->end(), w, w + 4);
            if (c.eat(',')) continue;
            if (!c.need(']')) return false;
            break;
        }
    if (count != 1) { *rows_ok = false; out->resize(out->size() + (count ? 0 : 4), 0); }
    return true;
}
// [[..],[..]]: rows of `row` words each, flattened (another row length clears *rows_ok)
bool u64_rows(Cur &c, size_t row, std::vector<u64> *out, bool *rows_ok) {
    if (!c.need('[')) return false;
    if (c.eat(']')) return true;
    for (;;) {
        const size_t before = out->size();
        if (!u64_list(c, out)) return false;
        if (out->size() - before != row) *rows_ok = false;
        if (c.eat(',')) continue;
        return c.need(']');
    }
}

bool parse_header(const char *text, size_t len, bool bn, ProofHeader *h) {
    Cur c{text, text + len};
    const bool ok = each_member(c, [&](const char *b, const char *e) {
        if (c.key_is(b, e, "params")) {
            if (!once(c, h->has_params)) return;
            bool got_hash = false;
            each_member(c, [&](const char *kb, const char *ke) {
                for (int i = 0; i < ProofHeader::NPARAM; i++)
                    if (c.key_is(kb, ke, PARAM_KEYS[i])) { if (once(c, h->has_param[i])) c.u64v(&h->param[i]); return; }
                if (c.key_is(kb, ke, "hash")) {
                    const char *sb, *se;
                    if (once(c, got_hash) && c.str(&sb, &se)) h->hash.assign(sb, se);
                    return;
                }
                c.skip_value();
            });
        } else if (c.key_is(b, e, "root32")) { if (once(c, h->has_root32)) c.u64v(&h->root32); }
        else if (c.key_is(b, e, "shift")) { if (once(c, h->has_shift)) c.u64v(&h->shift); }
        else if (c.key_is(b, e, "pow_nonce")) { if (once(c, h->has_nonce)) c.u64v(&h->nonce); }
        else if (c.key_is(b, e, "air_digest")) {
            const char *sb, *se;
            if (once(c, h->has_digest) && c.str(&sb, &se)) h->digest.assign(sb, se);
        } else if (c.key_is(b, e, "publics")) { if (once(c, h->has_pubs)) u64_list(c, &h->pubs); }
        else if (c.key_is(b, e, "roots")) {
            each_member(c, [&](const char *kb, const char *ke) {
                const int t = c.key_is(kb, ke, "trace") ? 0 : c.key_is(kb, ke, "stage2") ? 1 : c.key_is(kb, ke, "quotient") ? 2 : -1;
                if (t < 0) { c.skip_value(); return; }
                if (!once(c, h->has_root[t])) return;
                if (bn) fr_root(c, &h->root[t], &h->rows_ok);
                else if (u64_list(c, &h->root[t]) && h->root[t].size() != 4) h->rows_ok = false;
            });
        } else if (c.key_is(b, e, "evals")) {
            each_member(c, [&](const char *kb, const char *ke) {
                if (c.key_is(kb, ke, "z")) { if (once(c, h->has_z)) u64_rows(c, 3, &h->ev_z, &h->rows_ok); }
                else if (c.key_is(kb, ke, "zw")) { if (once(c, h->has_zw)) u64_rows(c, 3, &h->ev_zw, &h->rows_ok); }
                else c.skip_value();
            });
        } else if (c.key_is(b, e, "fri")) {
            each_member(c, [&](const char *kb, const char *ke) {
                if (c.key_is(kb, ke, "roots")) {
                    if (!once(c, h->has_fri_roots)) return;
                    if (!bn) { u64_rows(c, 4, &h->fri_roots, &h->rows_ok); return; }
                    if (!c.need('[') || c.eat(']')) return;
                    for (;;) {
                        if (!fr_root(c, &h->fri_roots, &h->rows_ok)) return;
                        if (c.eat(',')) continue;
                        c.need(']');
                        return;
                    }
                }
                else if (c.key_is(kb, ke, "final")) {
                    if (!once(c, h->has_final) || !c.need('[')) return;
                    if (c.eat(']')) return;
                    for (;;) {
                        if (h->final_l.size() >= 4) { c.ok = false; return; }
                        h->final_l.emplace_back();
                        if (!u64_list(c, &h->final_l.back())) return;
                        if (c.eat(',')) continue;
                        c.need(']');
                        return;
                    }
                } else c.skip_value();
            });
        } else if (c.key_is(b, e, "queries")) { if (once(c, h->has_queries)) c.skip_value(); }
        else c.skip_value();
    });
    c.ws();
    return ok && c.ok && c.p == c.end;
}

// in-place inverse transform of 2^lg values up to the factor 1 / 2^lg (the degree test looks for zeros only)
void intt_unscaled(std::vector<u64> &a, int lg, u64 root32) {
    const size_t n = (size_t)1 << lg;
    for (size_t i = 0, j = 0; i < n; i++) {
        if (i < j) std::swap(a[i], a[j]);
        size_t m = n >> 1;
        for (; m && (j & m); m >>= 1) j ^= m;
        j |= m;
    }
    for (int s = 1; s <= lg; s++) {
        const size_t half = (size_t)1 << (s - 1);
        const u64 w = gl_inv(gl_root(root32, s));
        for (size_t k = 0; k < n; k += 2 * half) {
            u64 t = 1;
            for (size_t j = 0; j < half; j++) {
                const u64 u = a[k + j], v = gl_mul(a[k + j + half], t);
                a[k + j] = gl_add(u, v);
                a[k + j + half] = gl_sub(u, v);
                t = gl_mul(t, w);
            }
        }
    }
}

struct VerifyParams { int logn, logb, fri_logf, fri_final_log, n_queries, pow_bits; uint32_t flags; int threads; u64 root32, shift; const HostPoseidon254 *H254; };      // H254: BN128-hash mode
struct ProgramInfo : ZpProgram { char digest_hex[17]; u64 digest_words[4]; };      // a statement as the verifiers hold it: the parsed blob and its digest

// one proof between the header checks and the verdict: what the query phase needs
struct Pending {
    int verdict = ZP_VERDICT_ACCEPT, where = -1;
    bool queries_live = false;                 // the header passed and there are openings to check
    std::vector<u64> qidx, index, values, paths, roots;      // roots: 4 words per tree (raw: a word >= p matches no digest)
    std::vector<int32_t> widths, depths, grp;  // per tree: leaf width, path entries, log2 of the rows a leaf holds (BN128 mode groups the committed trees' leaves)
    std::vector<u64> leaves;                   // per tree: its leaf count (a power of two)
    std::vector<size_t> voff, poff;            // where tree t's block starts in values / paths
    std::vector<std::pair<int, int>> sched;    // (log size of the layer, log fold factor)
    std::vector<u64> ev_z, ev_zw, final_raw;   // canonical evaluations; the final layer as the text has it, plane-major
    std::vector<e3> betas;
    e3 zeta, gamma;
    int final_log = 0, T = 0;
    size_t Wt = 0, Wall = 0;
    std::vector<uint8_t> open_ok, arith;       // per (query, tree): the opening hashes to its root; per (query, 0..n_fri): layer l's value / the final value is consistent
    size_t root0 = 0;                          // the slot of its first root in the batch's list
    // zp_aggregate_verify: the identity at zeta waits for the fixed columns of every header of the tree (one zp_program_fixed_eval_ext_batch per program)
    bool defer_identity = false, id_pending = false;
    std::vector<u64> id_pubchal;
    e3 id_alpha;
};

// the constraint identity at zeta: sum_k alpha^k C_k(zeta) = q(zeta) Z_H(zeta).  *v: ZP_VERDICT_ACCEPT or ZP_VERDICT_IDENTITY; the return code is
// not ZP_OK for a blob the evaluator refuses (the caller's mistake, not a rejected proof).  fixed_in: the fixed columns at zeta, when made elsewhere
int32_t identity_at_zeta(const ProgramInfo &pg, const VerifyParams &vp, const std::vector<u64> &pubchal, const e3 &alpha, const e3 &zeta, const std::vector<u64> &ev_z,
                         const std::vector<u64> &ev_zw, const uint64_t *fixed_in, int threads, int *v) {
    const int logn = vp.logn;
    const size_t Wt = pg.W + pg.W2, Q = pg.Q;
    std::vector<u64> cs(3 * pg.K);
    bool on_domain = false;
    *v = ZP_VERDICT_IDENTITY;
    const int32_t rc = program_eval_ext_impl(pg.words, pg.n_words, (const uint64_t *)pubchal.data(), (int32_t)(pg.n_pub + pg.n_chal), logn, vp.root32, (const uint64_t *)zeta.c,
                                             (const uint64_t *)ev_z.data(), (const uint64_t *)ev_zw.data(), (int32_t)Wt, (uint64_t *)cs.data(), (int32_t)pg.K, threads, nullptr, 0, &on_domain,
                                             fixed_in);
    if (rc != ZP_OK && !on_domain) return rc;
    if (rc != ZP_OK) return ZP_OK;             // zeta on the trace domain: nothing can be said at it
    e3 lhs = e3_base(0), ap = e3_base(1);
    for (size_t k = 0; k < pg.K; k++) { lhs = e3_add(lhs, e3_mul(ap, e3_make(cs[3 * k], cs[3 * k + 1], cs[3 * k + 2]))); ap = e3_mul(ap, alpha); }
    const e3 zN = e3_pow2k(zeta, logn), zh = e3_make(gl_sub(zN.c[0], 1), zN.c[1], zN.c[2]);
    const e3 zsN = e3_pow2k(e3_scale(zeta, gl_inv(vp.shift)), logn);
    auto mul_theta = [](const e3 &a) { return e3_make(a.c[2], gl_add(a.c[0], a.c[2]), a.c[1]); };      // theta^3 = theta + 1
    e3 q = e3_base(0), zpow = e3_base(1);
    for (size_t j = 0; j < Q; j++) {
        const u64 *p = &ev_z[3 * (Wt + 3 * j)];
        const e3 qj = e3_add(e3_add(e3_make(p[0], p[1], p[2]), mul_theta(e3_make(p[3], p[4], p[5]))), mul_theta(mul_theta(e3_make(p[6], p[7], p[8]))));
        q = e3_add(q, e3_mul(zpow, qj));
        zpow = e3_mul(zpow, zsN);
    }
    const e3 rhs = e3_mul(q, zh);
    if (memcmp(lhs.c, rhs.c, 24) == 0) *v = ZP_VERDICT_ACCEPT;
    return ZP_OK;
}

void fri_schedule(const VerifyParams &vp, std::vector<std::pair<int, int>> *sched, int *final_log) {
    int cur = vp.logn + vp.logb;
    const int stop = vp.fri_final_log + vp.logb;
    while (cur > stop) { const int f = vp.fri_logf < cur - stop ? vp.fri_logf : cur - stop; sched->push_back({cur, f}); cur -= f; }
    *final_log = cur;
}

// what opens a transcript: the statement and the parameters, then the public inputs themselves when there are at most 64 (PUBLICS_INLINE) -- ONE
// absorb (BN128 mode packs three values to an element per absorb); a longer vector follows as the root of its commitment
std::vector<u64> transcript_head(const ProgramInfo &pg, const VerifyParams &vp, const std::vector<u64> &pubs) {
    std::vector<u64> head = {(u64)vp.logn, (u64)vp.logb, (u64)pg.W, (u64)pg.W2, (u64)vp.fri_logf, (u64)vp.fri_final_log, (u64)vp.n_queries, (u64)vp.pow_bits, vp.root32, vp.shift,
                             pg.digest_words[0], pg.digest_words[1], pg.digest_words[2], pg.digest_words[3], (u64)pubs.size()};
    if (pubs.size() <= 64) head.insert(head.end(), pubs.begin(), pubs.end());
    return head;
}

// The schedule of a text's transcript: only the absorb and squeeze calls of the header phase below, in its order, on a parsed header -- what a
// PlanSponge records.  *digest_word: where in the plan's blocks the four words of the public inputs' commitment stand (more than 64 public inputs;
// zeros are planned, the caller writes the digest in).  false: the header lacks a member the walk needs, or has one of another size than the statement
// dictates, or (BN128 mode) a root >= r: no plan -- the header phase ends such a text MALFORMED / PARAMS / POW before much is hashed.
template <class M>
bool transcript_schedule(const ProofHeader &h, const ProgramInfo &pg, const VerifyParams &vp, PlanSponge<M> &tr, bool *long_pubs, size_t *digest_word) {
    const bool bn = vp.H254 != nullptr;
    const size_t Wt = pg.W + pg.W2, nq = (size_t)vp.n_queries;
    std::vector<std::pair<int, int>> sched;
    int final_log = 0;
    fri_schedule(vp, &sched, &final_log);
    auto root_ok = [&](const u64 *r) { return !bn || fr_is_canonical_u64(r); };
    if (!h.has_pubs || h.pubs.size() != pg.n_pub || !h.rows_ok || !h.has_root[0] || !h.has_root[2] || (pg.n_s2 && !h.has_root[1]) || !h.has_z || !h.has_zw ||
        h.ev_z.size() != 3 * (Wt + 3 * pg.Q) || h.ev_zw.size() != 3 * Wt || !h.has_fri_roots || !h.has_final || h.fri_roots.size() != 4 * sched.size() || h.final_l.size() != 3 ||
        (vp.pow_bits && !h.has_nonce))
        return false;
    if (!root_ok(h.root[0].data()) || !root_ok(h.root[2].data()) || (pg.n_s2 && !root_ok(h.root[1].data()))) return false;
    for (size_t l = 0; l < sched.size(); l++)
        if (!root_ok(&h.fri_roots[4 * l])) return false;
    for (int c = 0; c < 3; c++)
        if (h.final_l[c].size() != ((size_t)1 << final_log)) return false;
    std::vector<u64> out(nq > 4 ? nq : 4);
    const std::vector<u64> head = transcript_head(pg, vp, h.pubs);
    tr.absorb(head.data(), head.size());
    *long_pubs = h.pubs.size() > 64;
    if (*long_pubs) {
        const u64 zero[4] = {0, 0, 0, 0};
        *digest_word = tr.next_word();
        tr.absorb_root(zero);
    }
    tr.absorb_root(h.root[0].data());
    if (pg.n_s2) { tr.squeeze(3, out.data()); tr.absorb_root(h.root[1].data()); }
    tr.squeeze(3, out.data());                 // alpha
    tr.absorb_root(h.root[2].data());
    tr.squeeze(3, out.data());                 // zeta
    tr.absorb(h.ev_z.data(), h.ev_z.size());
    tr.absorb(h.ev_zw.data(), h.ev_zw.size());
    tr.squeeze(3, out.data());                 // gamma
    for (size_t l = 0; l < sched.size(); l++) { tr.absorb_root(&h.fri_roots[4 * l]); tr.squeeze(3, out.data()); }      // beta_l
    for (int c = 0; c < 3; c++) tr.absorb(h.final_l[c].data(), h.final_l[c].size());
    if (vp.pow_bits) { tr.squeeze(4, out.data()); const u64 nonce = h.nonce; tr.absorb(&nonce, 1); }
    tr.squeeze(nq, out.data());
    return true;
}

// what a caller that ran the transcripts of its texts elsewhere hands the header phase: the header it parsed, the sponge that replays the text's
// chain (NULL: the text got no plan and takes the host sponge), and the commitment of a long public-input vector when the device made it
struct HeaderAid { ProofHeader *parsed = nullptr; bool parsed_ok = false; Transcript *replay = nullptr; const u64 *pub_digest = nullptr; };

int32_t header_phase(const char *text, size_t len, const ProgramInfo &pg, const VerifyParams &vp, const HostPoseidon &H, Pending *pd, PublicSponge *ps = nullptr,
                     const HeaderAid *aid = nullptr) {
    auto verdict = [&](int v) { pd->verdict = v; return ZP_OK; };
    ProofHeader own;
    ProofHeader &h = aid && aid->parsed ? *aid->parsed : own;
    const bool bn = vp.H254 != nullptr;
    if (!(aid && aid->parsed ? aid->parsed_ok : parse_header(text, len, bn, &own))) return verdict(ZP_VERDICT_MALFORMED);
    // 1. parameters, domain, statement, counts
    const u64 want[ProofHeader::NPARAM] = {(u64)vp.logn, (u64)vp.logb, (u64)vp.fri_logf, (u64)vp.fri_final_log, (u64)vp.n_queries, (u64)vp.pow_bits};
    if (!h.has_params) return verdict(ZP_VERDICT_MALFORMED);
    for (int i = 0; i < ProofHeader::NPARAM; i++)
        if (!h.has_param[i] || h.param[i] != want[i]) return verdict(ZP_VERDICT_PARAMS);
    if (!bn && h.hash == "bn128") return ZP_ERR_UNSUPPORTED;
    if (h.hash != (bn ? "bn128" : "gl")) return verdict(ZP_VERDICT_PARAMS);
    if (!h.has_root32 || !h.has_shift || !h.has_digest || !h.has_pubs) return verdict(ZP_VERDICT_MALFORMED);
    if (h.root32 != vp.root32 || h.shift != vp.shift) return verdict(ZP_VERDICT_PARAMS);
    if (h.digest != pg.digest_hex) return verdict(ZP_VERDICT_PARAMS);
    if (pg.Q > ((size_t)1 << vp.logb)) return verdict(ZP_VERDICT_PARAMS);
    if (h.pubs.size() != pg.n_pub) return verdict(ZP_VERDICT_PARAMS);
    const int logn = vp.logn, logb = vp.logb, logm = logn + logb;
    const size_t W = pg.W, W2 = pg.W2, Wt = W + W2, Q = pg.Q, nq = (size_t)vp.n_queries;
    const u64 M = (u64)1 << logm;
    for (u64 &v : h.pubs) v = gl_canon(v);
    // the transcript (head and inline public inputs are ONE absorb: BN128 mode packs three values to an element per absorb)
    HostSponge tr_gl(H);
    static const HostPoseidon254 no_tables;
    HostSponge254 tr_bn(bn ? *vp.H254 : no_tables);
    // ps: the transcript is READ (an inner header of an aggregated proof); aid->replay: its permutations ran on the device, in the call's one chain launch
    Transcript &tr = ps ? (Transcript &)*ps : aid && aid->replay ? *aid->replay : bn ? (Transcript &)tr_bn : (Transcript &)tr_gl;
    auto root_ok = [&](const u64 *r) { return !bn || fr_is_canonical_u64(r); };      // "malformed BN128 root"
    {
        const std::vector<u64> head = transcript_head(pg, vp, h.pubs);
        tr.absorb(head.data(), head.size());
        if (h.pubs.size() > 64) {
            u64 dg[4];
            if (aid && aid->pub_digest) memcpy(dg, aid->pub_digest, 32);
            else if (bn) publics_digest_host254(*vp.H254, h.pubs, dg);
            else publics_digest_host(H, h.pubs, dg);
            tr.absorb_root(dg);
        }
    }
    if (!h.has_root[0] || !h.has_root[2] || !h.rows_ok) return verdict(ZP_VERDICT_MALFORMED);
    if (!root_ok(h.root[0].data()) || !root_ok(h.root[2].data()) || (pg.n_s2 && h.has_root[1] && !root_ok(h.root[1].data()))) return verdict(ZP_VERDICT_MALFORMED);
    tr.absorb_root(h.root[0].data());
    std::vector<u64> pubchal = h.pubs;
    if (pg.n_s2) {
        if (!h.has_root[1]) return verdict(ZP_VERDICT_MALFORMED);
        u64 ch[3];
        tr.squeeze(3, ch);
        pubchal.insert(pubchal.end(), ch, ch + 3);
        tr.absorb_root(h.root[1].data());
    }
    const e3 alpha = tr.challenge();
    tr.absorb_root(h.root[2].data());
    const e3 zeta = tr.challenge();
    if (!h.has_z || !h.has_zw || h.ev_z.size() != 3 * (Wt + 3 * Q) || h.ev_zw.size() != 3 * Wt) return verdict(ZP_VERDICT_MALFORMED);
    for (u64 &v : h.ev_z) v = gl_canon(v);
    for (u64 &v : h.ev_zw) v = gl_canon(v);
    tr.absorb(h.ev_z.data(), h.ev_z.size());
    tr.absorb(h.ev_zw.data(), h.ev_zw.size());
    const e3 gamma = tr.challenge();

    // 2. the constraint identity at zeta: sum_k alpha^k C_k(zeta) = q(zeta) Z_H(zeta) -- now, or once the caller has the fixed columns of all its headers
    pd->zeta = zeta; pd->gamma = gamma;
    if (pubchal.empty()) pubchal.push_back(0);
    if (pd->defer_identity) {
        pd->id_pending = true; pd->id_pubchal = pubchal; pd->id_alpha = alpha; pd->ev_z = h.ev_z; pd->ev_zw = h.ev_zw;
    } else {
        int v;
        const int32_t rc = identity_at_zeta(pg, vp, pubchal, alpha, zeta, h.ev_z, h.ev_zw, nullptr, vp.threads, &v);
        if (rc != ZP_OK) return rc;
        if (v != ZP_VERDICT_ACCEPT) return verdict(v);
    }

    // 3. the FRI transcript
    int cur = logm;
    const int stop = vp.fri_final_log + logb;
    while (cur > stop) { const int f = vp.fri_logf < cur - stop ? vp.fri_logf : cur - stop; pd->sched.push_back({cur, f}); cur -= f; }
    const int final_log = cur;
    pd->final_log = final_log;
    const size_t n_fri = pd->sched.size();
    if (!h.has_fri_roots || !h.has_final || h.fri_roots.size() != 4 * n_fri) return verdict(ZP_VERDICT_MALFORMED);
    for (size_t l = 0; l < n_fri; l++)
        if (!root_ok(&h.fri_roots[4 * l])) return verdict(ZP_VERDICT_MALFORMED);
    for (size_t l = 0; l < n_fri; l++) { tr.absorb_root(&h.fri_roots[4 * l]); pd->betas.push_back(tr.challenge()); }
    if (h.final_l.size() != 3) return verdict(ZP_VERDICT_MALFORMED);
    for (int c = 0; c < 3; c++)
        if (h.final_l[c].size() != ((size_t)1 << final_log)) return verdict(ZP_VERDICT_MALFORMED);
    for (int c = 0; c < 3; c++) tr.absorb(h.final_l[c].data(), h.final_l[c].size());
    // 4. grinding
    u64 pow_seed[4] = {0, 0, 0, 0};
    if (vp.pow_bits) {
        u64 seed[4];
        tr.squeeze(4, seed);
        memcpy(pow_seed, seed, 32);
        if (!h.has_nonce || h.nonce >= GL_P) return verdict(ZP_VERDICT_POW);
        u64 s[12] = {seed[0], seed[1], seed[2], seed[3], (u64)h.nonce, 0, 0, 0, 0, 0, 0, 0};
        if (!ps) {
            H.perm(s);
            if (s[0] >> (64 - vp.pow_bits)) return verdict(ZP_VERDICT_POW);
        }
        { const u64 nonce = h.nonce; tr.absorb(&nonce, 1); }
    }
    // 5. the indices the transcript dictates
    pd->qidx.resize(nq);
    tr.squeeze(nq, pd->qidx.data());
    for (u64 &v : pd->qidx) v &= M - 1;
    if (ps && vp.pow_bits) {                   // the grinding hash is the last permutation of a public transcript
        u64 seed[4];
        memcpy(seed, pow_seed, 32);
        if (ps->pow_digest0(seed, h.nonce) >> (64 - vp.pow_bits)) return verdict(ZP_VERDICT_POW);
    }
    const bool header_only = (vp.flags & ZP_VERIFY_HEADER_ONLY) != 0;
    size_t q_begin = 0, q_end = 0;
    int32_t nq_text = 0, has_s2 = 0, nf_text = 0, widths[48], depths[48];
    if (!header_only) {
        if (!zpi_proof_queries_scan || !zpi_proof_queries_parse) return ZP_ERR_UNSUPPORTED;
        if (!h.has_queries || zpi_proof_queries_scan(text, len, &q_begin, &q_end, &nq_text, &has_s2, &nf_text, widths, depths, 48, bn) != ZP_OK) return verdict(ZP_VERDICT_MALFORMED);
        if ((size_t)nq_text != nq) return verdict(ZP_VERDICT_INDICES);
        // every size below counts numbers that stand in the text; n_queries is the verifier's own
        const int T = 2 + has_s2 + nf_text;
        size_t nv = 0, np = 0;
        pd->widths.assign(widths, widths + T); pd->depths.assign(depths, depths + T);
        for (int t = 0; t < T; t++) { pd->voff.push_back(nv); pd->poff.push_back(np); nv += nq * (size_t)widths[t]; np += nq * (size_t)depths[t] * (bn ? 64 : 4); }
        pd->index.resize(nq); pd->values.resize(nv ? nv : 1); pd->paths.resize(np ? np : 1);
        if (zpi_proof_queries_parse(text, q_begin, q_end, nq_text, has_s2, nf_text, widths, depths, (uint64_t *)pd->index.data(), (uint64_t *)pd->values.data(),
                                    (uint64_t *)pd->paths.data(), bn) != ZP_OK)
            return verdict(ZP_VERDICT_MALFORMED);
        if (pd->index != pd->qidx) return verdict(ZP_VERDICT_INDICES);
        pd->T = T;
    }
    // 6. the final layer has degree < 2^(final_log - logb) on its coset (the unshift scales coefficient i by s^-i: zero stays zero)
    for (int c = 0; c < 3; c++) {
        std::vector<u64> cf(h.final_l[c]);
        for (u64 &v : cf) v = gl_canon(v);
        intt_unscaled(cf, final_log, vp.root32);
        for (size_t i = (size_t)1 << (final_log - logb); i < cf.size(); i++)
            if (cf[i]) return verdict(ZP_VERDICT_FINAL_DEGREE);
    }
    if (header_only) return verdict(ZP_VERDICT_ACCEPT);
    // the shape of the openings: trace, [stage 2], quotient, one per FRI layer.  BN128 mode: a committed leaf holds 2^g rows (stark/prover.py
    // bn128_rows_per_leaf_log: the largest g with width 2^g <= 56 values that leaves the tree 16 leaves), FRI leaves are not grouped, and a path has
    // ceil(log16) entries.  Checked before anything is hashed
    {
        const bool s2 = pg.n_s2 != 0;
        if ((has_s2 != 0) != s2 || (size_t)nf_text != n_fri) return verdict(ZP_VERDICT_MALFORMED);
        auto committed = [&](size_t w) {
            int g = 0;
            while (bn && (w << (g + 1)) <= 56 && g + 1 <= logm - 4) g++;
            pd->grp.push_back(g); pd->leaves.push_back(M >> g);
            return w << g;
        };
        std::vector<size_t> want_w = {committed(W)};
        if (s2) want_w.push_back(committed(W2));
        want_w.push_back(committed(3 * Q));
        for (auto &lf : pd->sched) { want_w.push_back((size_t)3 << lf.second); pd->grp.push_back(0); pd->leaves.push_back((u64)1 << (lf.first - lf.second)); }
        for (int t = 0; t < pd->T; t++) {
            int lg = 0;
            while (((u64)1 << lg) < pd->leaves[t]) lg++;
            if ((size_t)widths[t] != want_w[t] || depths[t] != (bn ? levels16(pd->leaves[t]) : lg)) return verdict(ZP_VERDICT_MALFORMED);
        }
    }
    pd->roots.insert(pd->roots.end(), h.root[0].begin(), h.root[0].end());
    if (pg.n_s2) pd->roots.insert(pd->roots.end(), h.root[1].begin(), h.root[1].end());
    pd->roots.insert(pd->roots.end(), h.root[2].begin(), h.root[2].end());
    pd->roots.insert(pd->roots.end(), h.fri_roots.begin(), h.fri_roots.end());
    pd->ev_z.swap(h.ev_z); pd->ev_zw.swap(h.ev_zw);
    for (int c = 0; c < 3; c++) pd->final_raw.insert(pd->final_raw.end(), h.final_l[c].begin(), h.final_l[c].end());
    pd->zeta = zeta; pd->gamma = gamma; pd->final_log = final_log; pd->Wt = Wt; pd->Wall = Wt + 3 * Q;
    pd->queries_live = true;
    return ZP_OK;
}

// the DEEP sum and every fold of query q: arith[q][l] = layer l's opened value is the previous fold (l = n_fri: the final layer's)
void query_arith(const Pending &pd, const VerifyParams &vp, const std::vector<e3> &gp, const std::vector<u64> &vals, size_t q, uint8_t *out) {
    const size_t n_fri = pd.sched.size(), Wt = pd.Wt, Wall = pd.Wall;
    const int logm = vp.logn + vp.logb, T = pd.T;
    const u64 j = pd.index[q], wM = gl_root(vp.root32, logm), x = gl_mul(vp.shift, gl_pow(wM, j));
    // columns in the order of the evaluations: trace, stage 2, quotient = trees 0 .. T - n_fri - 1
    e3 A = e3_base(0), B = e3_base(0);
    size_t k = 0;
    for (int t = 0; t < T - (int)n_fri; t++)
        for (int c = 0, g = pd.grp[t]; c < pd.widths[t] >> g; c++, k++) {
            // the queried row out of the 2^g rows of the leaf: column c of row j sits at c 2^g + j / (M / 2^g)  (g = 0: the leaf is the row)
            const u64 v = vals[pd.voff[t] + q * (size_t)pd.widths[t] + ((size_t)c << g) + (size_t)(j >> (logm - g))];
            A = e3_add(A, e3_mul(gp[k], e3_make(gl_sub(v, pd.ev_z[3 * k]), gl_neg(pd.ev_z[3 * k + 1]), gl_neg(pd.ev_z[3 * k + 2]))));
            if (k < Wt) B = e3_add(B, e3_mul(gp[Wall + k], e3_make(gl_sub(v, pd.ev_zw[3 * k]), gl_neg(pd.ev_zw[3 * k + 1]), gl_neg(pd.ev_zw[3 * k + 2]))));
        }
    const e3 zeta_w = e3_scale(pd.zeta, gl_root(vp.root32, vp.logn));
    e3 expect = e3_add(e3_mul(A, e3_inv(e3_make(gl_sub(x, pd.zeta.c[0]), gl_neg(pd.zeta.c[1]), gl_neg(pd.zeta.c[2])))),
                       e3_mul(B, e3_inv(e3_make(gl_sub(x, zeta_w.c[0]), gl_neg(zeta_w.c[1]), gl_neg(zeta_w.c[2])))));
    u64 pos = j, cur_shift = vp.shift;
    for (size_t l = 0; l < n_fri; l++) {
        const int lg = pd.sched[l].first, f = pd.sched[l].second, t = T - (int)n_fri + (int)l;
        const size_t F = (size_t)1 << f;
        const u64 row = pos & (((u64)1 << (lg - f)) - 1), k0 = pos >> (lg - f);
        const u64 *raw = &pd.values[pd.voff[t] + q * 3 * F], *lv = &vals[pd.voff[t] + q * 3 * F];
        out[l] = raw[k0] == expect.c[0] && raw[F + k0] == expect.c[1] && raw[2 * F + k0] == expect.c[2];
        // fold: c_j = (1 / F) x^-j sum_k v_k w_F^-jk, the next value sum_j beta^j c_j
        const u64 x_base = gl_mul(cur_shift, gl_pow(gl_root(vp.root32, lg), row)), winv = gl_inv(gl_root(vp.root32, f)), finv = gl_inv((u64)F), xinv = gl_inv(x_base);
        u64 wp[16];                            // fri_logf <= 4
        wp[0] = 1;
        for (size_t i = 1; i < F; i++) wp[i] = gl_mul(wp[i - 1], winv);
        e3 acc = e3_base(0), bp = e3_base(1);
        u64 s = finv;
        for (size_t jj = 0; jj < F; jj++) {
            u64 cj[3] = {0, 0, 0};
            for (size_t kk = 0; kk < F; kk++)
                for (int c = 0; c < 3; c++) cj[c] = gl_add(cj[c], gl_mul(lv[c * F + kk], wp[(jj * kk) & (F - 1)]));
            acc = e3_add(acc, e3_mul(e3_scale(e3_make(cj[0], cj[1], cj[2]), s), bp));
            bp = e3_mul(bp, pd.betas[l]);
            s = gl_mul(s, xinv);
        }
        expect = acc;
        pos = row;
        cur_shift = gl_pow(cur_shift, (u64)F);
    }
    const size_t nf = (size_t)1 << pd.final_log;
    out[n_fri] = pd.final_raw[pos] == expect.c[0] && pd.final_raw[nf + pos] == expect.c[1] && pd.final_raw[2 * nf + pos] == expect.c[2];
}

template <class F>
void spread(size_t n, int threads, F f) {              // f(i) for i < n over `threads` host threads (as zp_program_eval_ext spreads its columns)
    const unsigned nt = n < 8 ? 1 : zpi_host_threads(threads);
    zpi_over_threads(nt, [&](unsigned t) noexcept { for (size_t i = t; i < n; i += nt) f(i); });
}

// the first failing check in the protocol's order: per query the trace, quotient and stage-2 openings, then per layer its opening and its
// consistency with the previous fold, then the last fold against the final layer
void scan_verdict(Pending *pd, const VerifyParams &vp, bool has_s2) {
    const size_t nq = (size_t)vp.n_queries, n_fri = pd->sched.size();
    const int T = pd->T, tq = has_s2 ? 2 : 1;
    for (size_t q = 0; q < nq; q++) {
        const uint8_t *ok = &pd->open_ok[q * T], *ar = &pd->arith[q * (n_fri + 1)];
        int v = ZP_VERDICT_ACCEPT;
        if (!ok[0] || !ok[tq] || (has_s2 && !ok[1])) v = ZP_VERDICT_OPENING;
        for (size_t l = 0; l < n_fri && v == ZP_VERDICT_ACCEPT; l++) v = !ok[tq + 1 + l] ? ZP_VERDICT_OPENING : !ar[l] ? ZP_VERDICT_FRI : ZP_VERDICT_ACCEPT;
        if (v == ZP_VERDICT_ACCEPT && !ar[n_fri]) v = ZP_VERDICT_FRI;
        if (v != ZP_VERDICT_ACCEPT) { pd->verdict = v; pd->where = (int)q; return; }
    }
}

// the verifier's own parameters, and a statement: what the header phase needs to know of a program blob (false: not a program a STARK here is over)
bool params_in_range(const VerifyParams &vp) {
    return !(vp.logn < 1 || vp.logb < 1 || vp.logn + vp.logb > 30 || vp.fri_logf < 1 || vp.fri_logf > 4 || vp.fri_final_log < 0 || vp.fri_final_log >= vp.logn || vp.n_queries < 1 ||
             vp.n_queries > 4096 || vp.pow_bits < 0 || vp.pow_bits > 40 || (vp.flags & ~(uint32_t)(ZP_VERIFY_HEADER_ONLY | ZP_VERIFY_TRUST_OPENINGS)));
}
bool program_info(const uint64_t *h_program, size_t program_words, ProgramInfo *out) {
    ProgramInfo &pg = *out;
    if (!zpi_program_read(h_program, program_words, ZPG_VERIFY, &pg, nullptr)) return false;
    uint8_t dg[32];
    Sha256::digest((const uint8_t *)h_program, program_words * 8, dg);
    for (int i = 0; i < 8; i++) snprintf(pg.digest_hex + 2 * i, 3, "%02x", dg[i]);
    for (int i = 0; i < 4; i++) { u64 w = 0; for (int b = 7; b >= 0; b--) w = (w << 8) | dg[8 * i + b]; pg.digest_words[i] = w % GL_P; }
    return true;
}

// The query phase of every proof whose header passed: the openings of all of them in ONE launch on a ctx (here on the host without one), the DEEP sum
// and the folds at every query, then the first failing check per proof
int32_t queries_phase(zp_ctx *ctx, const VerifyParams &vp, const HostPoseidon &H, std::vector<Pending> &pend, bool has_s2) {
    const bool trust = (vp.flags & ZP_VERIFY_TRUST_OPENINGS) != 0, bn = vp.H254 != nullptr;
    const size_t nq = (size_t)vp.n_queries;
    // the openings of every proof that got this far, tree by tree (a wave of the device kernel then holds one tree shape), and their arithmetic
    std::vector<std::vector<u64>> canon(pend.size());
    std::vector<ZpOpening> ops;
    std::vector<u64> roots;
    int Tmax = 0;
    for (size_t i = 0; i < pend.size(); i++) {
        Pending &pd = pend[i];
        if (!pd.queries_live) continue;
        canon[i] = pd.values;
        for (u64 &v : canon[i]) v = gl_canon(v);
        if (!bn) for (u64 &v : pd.paths) v = gl_canon(v);      // (a BN128 path word is compared, never reduced: one >= r equals nothing)
        pd.open_ok.assign(nq * pd.T, 1);
        pd.arith.assign(nq * (pd.sched.size() + 1), 0);
        Tmax = pd.T > Tmax ? pd.T : Tmax;
    }
    if (trust) {
        // the opened values as given: only their range is checked (a recursion STARK vouches for the paths)
        for (Pending &pd : pend)
            for (int t = 0; pd.queries_live && t < pd.T; t++)
                for (size_t q = 0; q < nq; q++)
                    for (int c = 0; c < pd.widths[t]; c++)
                        if (pd.values[pd.voff[t] + q * (size_t)pd.widths[t] + c] >= GL_P) pd.open_ok[q * pd.T + t] = 0;
    } else {
        for (int t = 0; t < Tmax; t++)
            for (size_t i = 0; i < pend.size(); i++) {
                Pending &pd = pend[i];
                if (!pd.queries_live) continue;
                if (t == 0) { pd.root0 = roots.size() / 4; roots.insert(roots.end(), pd.roots.begin(), pd.roots.end()); }
                for (size_t q = 0; q < nq; q++) {
                    // the leaf of tree t that query q opens: a tree of 2^m leaves (a FRI layer, a grouped commitment) is opened at the low m bits of the index.
                    // BN128 mode hashes the opened values as the text has them (the checker packs them unreduced)
                    const std::vector<u64> &hv = bn ? pd.values : canon[i];
                    ops.push_back({&hv[pd.voff[t] + q * (size_t)pd.widths[t]], &pd.paths[pd.poff[t] + q * (size_t)pd.depths[t] * (bn ? 64 : 4)], pd.index[q] & (pd.leaves[t] - 1),
                                   (uint32_t)pd.widths[t], (uint32_t)pd.depths[t], (uint32_t)(pd.root0 + t), pd.leaves[t]});
                }
            }
        std::vector<uint8_t> ok(ops.size() ? ops.size() : 1);
        if (ctx && !ops.empty()) {
            const auto device = bn ? zpi_merkle16_verify_openings_bn254 : zpi_merkle_verify_openings;
            if (!device) { ctx->err = "this build has no device side"; return ZP_ERR_UNSUPPORTED; }
            ZP_TRY(device(ctx, ops.data(), ops.size(), roots.data(), roots.size() / 4, ok.data()));
        } else {
            spread(ops.size(), vp.threads, [&](size_t o) {
                const u64 *root = &roots[4 * (size_t)ops[o].root_slot];
                ok[o] = bn ? vp.H254->opening_ok(ops[o], root) : H.opening_ok(ops[o], root);
            });
        }
        size_t o = 0;
        for (int t = 0; t < Tmax; t++)
            for (Pending &pd : pend)
                for (size_t q = 0; pd.queries_live && q < nq; q++) pd.open_ok[q * pd.T + t] = ok[o++];
    }
    for (size_t i = 0; i < pend.size(); i++) {
        Pending &pd = pend[i];
        if (!pd.queries_live) continue;
        std::vector<e3> gp(pd.Wall + pd.Wt);
        e3 g = e3_base(1);
        for (e3 &x : gp) { x = g; g = e3_mul(g, pd.gamma); }
        spread(nq, vp.threads, [&](size_t q) { query_arith(pd, vp, gp, canon[i], q, &pd.arith[q * (pd.sched.size() + 1)]); });
        scan_verdict(&pd, vp, has_s2);
    }
    return ZP_OK;
}

// ---- The transcripts of a call on the device ("verify_chain_dev"; ctx.hpp).  Every text of the call is parsed and its schedule recorded as one chain;
// the commitments of the long public-input vectors are made with the prover's tree kernels and written into their blocks (first synchronisation); ALL
// chains of the call run in ONE launch of the mode's chain kernel (second synchronisation); the header phases then replay them.  A text that gets no
// plan takes the host sponge (counted: zp_verify_counters).  Verdicts, *where, indices and error codes are the host path's word for word: the device
// path moves permutations and nothing else.
bool chains_on_device(const zp_ctx *ctx, bool bn) {
    if (!ctx || ctx->tune_verify_chain_dev == 0) return false;
    (void)bn;
    return ctx->tune_verify_chain_dev == 2;            // the default leaves both modes on the host: neither beat the parent at every measured batch size (ctx.hpp)
}
struct TextPlan {
    ProofHeader h;
    bool parsed_ok = false, planned = false, long_pubs = false;
    size_t chain = 0, digest_word = 0;
    u64 digest[4] = {0, 0, 0, 0};
};
struct PlanItem { const char *text; size_t len; const ProgramInfo *pg; const VerifyParams *vp; };
struct DeviceTranscripts {
    bool on = false, bn = false;
    ChainPlan cp;
    std::vector<TextPlan> tp;

    template <class M>
    int32_t run_mode(zp_ctx *ctx, const std::vector<PlanItem> &items) {
        const auto chains = bn ? zpi_poseidon254_chains_host : zpi_poseidon_chains_host;
        const auto digests = bn ? zpi_publics_digests_bn254 : zpi_publics_digests;
        if (!chains || !digests) { ctx->err = "this build has no device side"; return ZP_ERR_UNSUPPORTED; }
        tp = std::vector<TextPlan>(items.size());
        std::vector<const std::vector<u64> *> longs;
        std::vector<size_t> who;
        for (size_t i = 0; i < items.size(); i++) {
            TextPlan &t = tp[i];
            t.parsed_ok = parse_header(items[i].text, items[i].len, bn, &t.h);
            if (t.parsed_ok) {
                PlanSponge<M> ps(cp);
                t.planned = transcript_schedule(t.h, *items[i].pg, *items[i].vp, ps, &t.long_pubs, &t.digest_word);      // (false: nothing was recorded)
                if (t.planned) { t.chain = cp.first.size() - 1; ps.close(); }
            }
            if (!t.planned) { ctx->verify_counters[3]++; continue; }
            if (t.long_pubs) {
                for (u64 &v : t.h.pubs) v = gl_canon(v);
                longs.push_back(&t.h.pubs); who.push_back(i);
            }
        }
        if (!longs.empty()) {
            std::vector<u64> dg(4 * longs.size());
            ZP_TRY(digests(ctx, longs, dg.data()));
            for (size_t k = 0; k < who.size(); k++) {
                memcpy(tp[who[k]].digest, &dg[4 * k], 32);
                memcpy(&cp.blocks[tp[who[k]].digest_word], &dg[4 * k], 32);
            }
            ctx->verify_counters[2] += longs.size();
        }
        if (cp.absorb.empty()) return ZP_OK;
        if (cp.absorb.size() >= ((size_t)1 << 31)) { ctx->err = "too many transcript steps in one call"; return ZP_ERR_ARG; }
        cp.rates.resize(cp.blocks.size());
        return chains(ctx, cp.blocks.data(), cp.absorb.data(), cp.first.data(), (int)(cp.first.size() - 1), cp.rates.data());
    }
    int32_t run(zp_ctx *ctx, bool bn_mode, const std::vector<PlanItem> &items) {
        on = true; bn = bn_mode;
        return bn ? run_mode<BnMode>(ctx, items) : run_mode<GlMode>(ctx, items);
    }
    // the header phase of text i on its chain
    int32_t header(size_t i, const char *text, size_t len, const ProgramInfo &pg, const VerifyParams &vp, const HostPoseidon &H, Pending *pd) {
        TextPlan &t = tp[i];
        HeaderAid aid;
        aid.parsed = &t.h; aid.parsed_ok = t.parsed_ok;
        if (!t.planned) return header_phase(text, len, pg, vp, H, pd, nullptr, &aid);
        if (t.long_pubs) aid.pub_digest = t.digest;
        ReplaySponge<GlMode> gl(cp, t.chain);
        ReplaySponge<BnMode> b254(cp, t.chain);
        aid.replay = bn ? (Transcript *)&b254 : (Transcript *)&gl;
        return header_phase(text, len, pg, vp, H, pd, nullptr, &aid);
    }
};

int32_t verify_batch_impl(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const char *const *proofs, const size_t *lens, int32_t n_proofs, VerifyParams vp,
                          int32_t *verdicts, int32_t *where, uint64_t *h_indices) {
    if (!h_program || !proofs || !lens || !verdicts || n_proofs < 1 || n_proofs > (1 << 20)) return ZP_ERR_ARG;
    for (int32_t i = 0; i < n_proofs; i++)
        if (!proofs[i]) return ZP_ERR_ARG;
    if (!params_in_range(vp)) return ZP_ERR_ARG;
    ProgramInfo pg;
    if (!program_info(h_program, program_words, &pg)) return ZP_ERR_ARG;
    vp.root32 = ctx ? ctx->root32 : ZP_ROOT32_DEFAULT;
    vp.shift = ctx ? ctx->coset_shift : ZP_SHIFT_DEFAULT;
    const HostPoseidon H = {ctx ? ctx->h_rc : (const u64 *)ZP_POSEIDON_DEFAULT_RC, ctx ? ctx->h_mds : (const u64 *)ZP_POSEIDON_DEFAULT_MDS};
    const size_t nq = (size_t)vp.n_queries;

    std::vector<Pending> pend((size_t)n_proofs);
    std::vector<int32_t> hrc((size_t)n_proofs, ZP_OK);
    // the transcripts of all texts as one chain launch, where they go to the device
    DeviceTranscripts dt;
    if (chains_on_device(ctx, vp.H254 != nullptr)) {
        std::vector<PlanItem> items((size_t)n_proofs);
        for (int32_t i = 0; i < n_proofs; i++) items[i] = {proofs[i], lens[i], &pg, &vp};
        ZP_TRY(dt.run(ctx, vp.H254 != nullptr, items));
    }
    // headers: a transcript is a serial chain, proofs are independent
    spread((size_t)n_proofs, n_proofs > 1 ? vp.threads : 1, [&](size_t i) {
        try {
            VerifyParams one = vp;
            if (n_proofs > 1) one.threads = 1;
            hrc[i] = dt.on ? dt.header(i, proofs[i], lens[i], pg, one, H, &pend[i]) : header_phase(proofs[i], lens[i], pg, one, H, &pend[i]);
        }
        catch (const std::bad_alloc &) { hrc[i] = ZP_ERR_NOMEM; }
        catch (...) { hrc[i] = ZP_ERR_INTERNAL; }
    });
    for (int32_t r : hrc)
        if (r != ZP_OK) {
            if (ctx) ctx->err = r == ZP_ERR_UNSUPPORTED ? "a proof in BN128-hash mode handed to the Goldilocks-mode call (or a build without the openings parser)"
                              : r == ZP_ERR_INTERNAL ? "internal error in a header phase (a transcript replay that left its plan)" : "the program blob could not be evaluated at the proof's point";
            return r;
        }

    ZP_TRY(queries_phase(ctx, vp, H, pend, pg.n_s2 != 0));
    for (int32_t i = 0; i < n_proofs; i++) verdicts[i] = pend[i].verdict;
    if (where) *where = pend[0].where;
    // the indices exist once the transcript got to them: an accepted proof, or one rejected by the check on the indices or a later one
    if (h_indices && (pend[0].verdict == ZP_VERDICT_ACCEPT || pend[0].verdict >= ZP_VERDICT_INDICES)) memcpy(h_indices, pend[0].qidx.data(), 8 * nq);
    return ZP_OK;
}

template <class Body>
int32_t verify_guarded(zp_ctx *ctx, Body body) {      // no exception crosses the ABI (the guarded() of csrc/prove.hip, for a ctx that may be NULL)
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try { if (ctx) ctx->err = "out of host memory while verifying"; } catch (...) {}
        return ZP_ERR_NOMEM;
    } catch (const std::exception &e) {
        try { if (ctx) ctx->err = std::string("internal error: ") + e.what(); } catch (...) {}
        return ZP_ERR_INTERNAL;
    } catch (...) {
        return ZP_ERR_INTERNAL;
    }
}

// the t = 17 tables of a BN128-mode call: with a ctx the ones installed on its device (zp_set_poseidon_bn254; none: the error zp_stark_prove_bn128
// gives), with ctx = NULL the caller's, in the layout of zp_set_poseidon_bn254
int32_t tables254(zp_ctx *ctx, int32_t rp, const uint64_t *h_rc, const uint64_t *h_mds, HostPoseidon254 *H) {
    if (ctx) {
        ZP_ARG(ctx, !h_rc && !h_mds, "with a ctx the installed t = 17 tables are used: pass h_rc and h_mds as NULL");
        if (!zpi_p254_host_tables) { ctx->err = "this build has no device side"; return ZP_ERR_UNSUPPORTED; }
        return zpi_p254_host_tables(ctx, &H->rc, &H->mds, &H->rp);
    }
    if (rp < 1 || rp > 128 || !h_rc || !h_mds) return ZP_ERR_ARG;
    const size_t nrc = (size_t)(8 + rp) * 17, nm = 17 * 17;
    H->rp = rp;
    H->rc.resize(nrc * 9); H->mds.resize(nm * 9);
    for (size_t i = 0; i < nrc + nm; i++) {
        const uint64_t *src = i < nrc ? h_rc + 4 * i : h_mds + 4 * (i - nrc);
        const u64 w[4] = {src[0], src[1], src[2], src[3]};
        if (!fr_is_canonical_u64(w)) return ZP_ERR_ARG;
        const fr m = fr_to_mont(fr_from_u64(w));
        memcpy(i < nrc ? &H->rc[9 * i] : &H->mds[9 * (i - nrc)], m.l, 36);
    }
    return ZP_OK;
}

// ================================================================================================================================
// The verifier of AGGREGATED proofs behind zp_aggregate_verify / zp_aggregate_verify_batch: what GenAggregatedProof returns and GenFinalProof takes.
//   text = {"shape"?, "inner": [header ...], "children"?: [node ...], "stark": proof}      node = {"shape", "inner", "children"?}
// A node's "inner" are HEADERS (no "queries").  A STARK over the verifier AIR of the node's shape vouches for them: the outer "stark" for the top
// node, header i of the parent for child i -- its public inputs are then facts.  Accepting means every chunk proof at the leaves verifies:
//   the outer STARK verifies under the statement of the top shape (header and query phases above; Goldilocks-hash mode);
//   per node, natively, what needs no opening: every header passes the header phase with its transcript READ off the vouching public inputs
//   (PublicSponge; the stream used up exactly), and those public inputs are exactly, in order: roots | leaf index of every (slot, proof, tree) |
//   transcripts | the arithmetic constants per proof | the final-layer value at every slot's position.
// The protocol is stark/verifier_air.py's and stark/prover.py's; the checker's independent statement is oracle/aggregate_verify.py (verify_tree).
// Order of the checks (the first failing one decides): the grammar of the whole text; its depth (more than AGG_MAX_DEPTH levels of nodes: TREE); the outer STARK (header, identity, queries); then the nodes
// depth-first in text order (pre-order number 0 = the top node), per node: its structure (TREE / PARAMS), its headers in order (each: header phase,
// identity), the length of the transcript section (TRANSCRIPT), the other sections (PUBLICS).
// The identity at zeta of EVERY header of every text of a call takes its fixed columns from one zp_program_fixed_eval_ext_batch per distinct
// statement: the challenges come from the public stream, so all (program, public inputs, zeta) are known before anything is evaluated.
enum { SHAPE_KEYS = 13, AGG_MAX_DEPTH = 8 };
const char *const SHAPE_KEY[SHAPE_KEYS] = {"logn", "logb", "W", "W2", "Wq", "n_queries", "fri_logf", "fri_final_log", "n_proofs", "n_pub_inner", "pow_bits", "root32", "shift"};
const u64 SHAPE_MAX[SHAPE_KEYS] = {30, 8, 4096, 4096, 64, 4096, 4, 16, 64, 1u << 24, 64, GL_P - 1, GL_P - 1};

// a shape dictionary (stark/verifier_air.py Shape.from_dict: every member bounded before it sizes anything).  The return value is the GRAMMAR
// (an object of exactly these members, each a non-negative integer < 2^64, each once); *in_range the bounds
bool parse_shape(Cur &c, u64 *v, bool *in_range) {
    bool got[SHAPE_KEYS] = {};
    const bool ok = each_member(c, [&](const char *b, const char *e) {
        for (int i = 0; i < SHAPE_KEYS; i++)
            if (c.key_is(b, e, SHAPE_KEY[i])) { if (once(c, got[i])) { uint64_t x = 0; c.u64v(&x); v[i] = x; } return; }
        c.ok = false;
    });
    if (!ok || !c.ok) return false;
    *in_range = true;
    for (int i = 0; i < SHAPE_KEYS; i++)
        if (!got[i] || v[i] > SHAPE_MAX[i]) *in_range = false;
    if (v[0] < 1 || v[1] < 1 || v[2] < 1 || v[4] < 1 || v[5] < 1 || v[6] < 1 || v[8] < 1 || v[0] + v[1] > 32 || v[11] < 2 || v[12] < 1) *in_range = false;
    if (v[0] + v[1] <= v[7] + v[1] || v[0] + v[1] < 2) *in_range = false;      // no committed FRI layer
    return true;
}

struct Span { const char *p; size_t n; };
struct AggNode {
    bool has_shape = false, shape_ok = false, has_inner = false, has_children = false, has_stark = false, too_deep = false;
    u64 shape[SHAPE_KEYS] = {};
    std::vector<Span> inner;
    std::vector<AggNode> kids;
    Span stark = {nullptr, 0};
};

bool object_span(Cur &c, Span *out) {
    c.ws();
    const char *b = c.p;
    if (!c.peek('{')) return c.ok = false;
    c.skip_value();
    *out = {b, (size_t)(c.p - b)};
    return c.ok;
}

// depth: 1 for the top node.  A node at AGG_MAX_DEPTH that has children is marked too_deep and its children are skipped, not walked
bool parse_node(Cur &c, AggNode *nd, int depth) {
    const bool ok = each_member(c, [&](const char *b, const char *e) {
        if (c.key_is(b, e, "shape")) { if (once(c, nd->has_shape)) parse_shape(c, nd->shape, &nd->shape_ok); }
        else if (c.key_is(b, e, "stark")) { if (once(c, nd->has_stark)) object_span(c, &nd->stark); }
        else if (c.key_is(b, e, "inner")) {
            if (!once(c, nd->has_inner) || !c.need('[') || c.eat(']')) return;
            for (;;) {
                Span sp;
                if (!object_span(c, &sp)) return;
                nd->inner.push_back(sp);
                if (c.eat(',')) continue;
                c.need(']');
                return;
            }
        } else if (c.key_is(b, e, "children")) {
            if (!once(c, nd->has_children) || !c.need('[') || c.eat(']')) return;
            for (;;) {
                if (depth >= AGG_MAX_DEPTH) { Span sp; nd->too_deep = true; if (!object_span(c, &sp)) return; }
                else { nd->kids.emplace_back(); if (!parse_node(c, &nd->kids.back(), depth + 1)) { c.ok = false; return; } }
                if (c.eat(',')) continue;
                c.need(']');
                return;
            }
        } else c.skip_value();
    });
    return ok && c.ok;
}

bool too_deep(const AggNode &nd) {
    if (nd.too_deep) return true;
    for (const AggNode &k : nd.kids)
        if (too_deep(k)) return true;
    return false;
}

struct AggStmt { bool leaf = false; u64 shape[SHAPE_KEYS] = {}; ProgramInfo pg; VerifyParams vp; size_t n_slots = 0; };

int find_stmt(const std::vector<AggStmt> &st, const u64 *shape) {      // shape = NULL: the leaf statement
    for (size_t i = 0; i < st.size(); i++)
        if (shape ? !st[i].leaf && memcmp(st[i].shape, shape, sizeof st[i].shape) == 0 : st[i].leaf) return (int)i;
    return -1;
}

struct HeaderJob {
    Span text = {nullptr, 0};
    int stmt = -1;
    ProofHeader raw;                           // the header as the text has it (public inputs, roots, final layer: compared unreduced)
    Pending pd;
    int id_verdict = ZP_VERDICT_ACCEPT;
    int32_t rc = ZP_OK;
};
struct NodeJob {
    const AggNode *nd = nullptr;
    int stmt_own = -1, stmt_inner = -1;
    const std::vector<u64> *pubs = nullptr;    // the vouching STARK's public inputs
    std::vector<HeaderJob> hdr;
    int verdict = ZP_VERDICT_ACCEPT;           // decided while planning (structure): the node is not run
    int post_verdict = ZP_VERDICT_ACCEPT;      // after its headers: the sections of the public inputs
    int32_t rc = ZP_OK;
};
struct TextJob {
    AggNode top;
    int verdict = ZP_VERDICT_ACCEPT, where = -1, top_stmt = -1;
    HeaderJob outer;
    std::vector<NodeJob *> nodes;              // pre-order
    ~TextJob() { for (NodeJob *n : nodes) delete n; }
    TextJob() = default;
    TextJob(const TextJob &) = delete;
    TextJob &operator=(const TextJob &) = delete;
};

// the structure of a node and of everything below it, pre-order; nothing is hashed or evaluated here
void plan_node(TextJob *tj, const AggNode &nd, const std::vector<u64> *pubs, const std::vector<AggStmt> &st, bool top) {
    NodeJob *nj = new NodeJob;
    tj->nodes.push_back(nj);
    nj->nd = &nd; nj->pubs = pubs;
    auto stop = [&](int v) { nj->verdict = v; };
    if (!nd.has_inner) return stop(ZP_VERDICT_MALFORMED);
    if (nd.has_shape && !nd.shape_ok) return stop(ZP_VERDICT_MALFORMED);
    if (nd.inner.empty() || (!nd.has_shape && !top)) return stop(ZP_VERDICT_TREE);
    nj->hdr.resize(nd.inner.size());
    for (size_t i = 0; i < nd.inner.size(); i++) {
        nj->hdr[i].text = nd.inner[i];
        if (!parse_header(nd.inner[i].p, nd.inner[i].n, false, &nj->hdr[i].raw)) return stop(ZP_VERDICT_MALFORMED);
    }
    for (const HeaderJob &h : nj->hdr)
        if (h.raw.has_queries) return stop(ZP_VERDICT_TREE);      // an aggregated proof carries no openings of its inner proofs
    if (!nd.kids.empty()) {
        if (nd.kids.size() != nd.inner.size()) return stop(ZP_VERDICT_TREE);
        for (const AggNode &k : nd.kids) {
            if (k.has_shape && !k.shape_ok) return stop(ZP_VERDICT_MALFORMED);
            if (!k.has_shape || memcmp(k.shape, nd.kids[0].shape, sizeof k.shape) != 0) return stop(ZP_VERDICT_TREE);
        }
    }
    // the statement of this node's shape gives the query slots of the vouching trace; a node without a shape (a level-1 text) takes the first
    // statement of the table that is not the leaf's
    if (nd.has_shape) nj->stmt_own = find_stmt(st, nd.shape);
    else for (size_t i = 0; i < st.size() && nj->stmt_own < 0; i++) if (!st[i].leaf) nj->stmt_own = (int)i;
    nj->stmt_inner = nd.kids.empty() ? find_stmt(st, nullptr) : find_stmt(st, nd.kids[0].shape);
    if (nj->stmt_own < 0 || nj->stmt_inner < 0) return stop(ZP_VERDICT_PARAMS);
    for (HeaderJob &h : nj->hdr) h.stmt = nj->stmt_inner;
    for (size_t i = 0; i < nd.kids.size(); i++) plan_node(tj, nd.kids[i], &nj->hdr[i].raw.pubs, st, false);
}

// what the verifier AIR takes as public per inner proof for its arithmetic constraints (stark/verifier_air.py arith_publics): g^1..g^8 with
// g = 1 / gamma; gamma^(Wall-1); gamma^(Wall+Wt-1); E_z; E_zw; zeta; zeta w; beta_l^j (1 <= j < 2^f) for every committed layer
void arithmetic_publics(const Pending &pd, const ProgramInfo &pg, const VerifyParams &vp, std::vector<u64> *out) {
    auto put = [&](const e3 &x) { out->insert(out->end(), x.c, x.c + 3); };
    const e3 g = e3_inv(pd.gamma);
    e3 cur = e3_base(1);
    for (int i = 0; i < 8; i++) { cur = e3_mul(cur, g); put(cur); }
    const size_t Wt = pg.W + pg.W2, Wall = Wt + 3 * pg.Q;
    std::vector<e3> gp(Wall + Wt);
    cur = e3_base(1);
    for (e3 &x : gp) { x = cur; cur = e3_mul(cur, pd.gamma); }
    e3 eza = e3_base(0), ezb = e3_base(0);
    for (size_t k = 0; k < Wall; k++) eza = e3_add(eza, e3_mul(gp[k], e3_make(pd.ev_z[3 * k], pd.ev_z[3 * k + 1], pd.ev_z[3 * k + 2])));
    for (size_t k = 0; k < Wt; k++) ezb = e3_add(ezb, e3_mul(gp[Wall + k], e3_make(pd.ev_zw[3 * k], pd.ev_zw[3 * k + 1], pd.ev_zw[3 * k + 2])));
    put(gp[Wall - 1]); put(gp[Wall + Wt - 1]); put(eza); put(ezb); put(pd.zeta); put(e3_scale(pd.zeta, gl_root(vp.root32, vp.logn)));
    for (size_t l = 0; l < pd.sched.size(); l++) {
        cur = e3_base(1);
        for (int j = 1; j < (1 << pd.sched[l].second); j++) { cur = e3_mul(cur, pd.betas[l]); put(cur); }
    }
}

// the headers of one node against the vouching public inputs; identities are left pending
void run_node(NodeJob *nj, const std::vector<AggStmt> &st, const HostPoseidon &H) {
    const AggStmt &S = st[nj->stmt_inner];
    const std::vector<u64> &pubs = *nj->pubs;
    std::vector<std::pair<int, int>> sched;
    int final_log = 0;
    fri_schedule(S.vp, &sched, &final_log);
    if (sched.empty()) { nj->verdict = ZP_VERDICT_PARAMS; return; }      // inner proofs without a committed FRI layer are not aggregated
    const size_t n_in = nj->hdr.size(), n_slots = st[nj->stmt_own].n_slots, T = 2 + (S.pg.W2 ? 1 : 0) + sched.size(), nq = (size_t)S.vp.n_queries;
    size_t n_arith = 42;
    for (auto &lf : sched) n_arith += 3 * (((size_t)1 << lf.second) - 1);
    const size_t n_merkle = n_in * T * 4 + n_slots * n_in * T, n_tail = n_in * n_arith + n_slots * n_in * 3;
    if (pubs.size() < n_merkle + n_tail) { nj->verdict = ZP_VERDICT_PUBLICS; return; }
    PublicSponge ps(pubs.data() + n_merkle, pubs.size() - n_merkle - n_tail);
    VerifyParams vp = S.vp;
    vp.flags = ZP_VERIFY_HEADER_ONLY;
    vp.threads = 1;
    for (HeaderJob &h : nj->hdr) {
        ps.reset();                            // a fresh queue per proof on the one stream
        h.pd.defer_identity = true;
        try { h.rc = header_phase(h.text.p, h.text.n, S.pg, vp, H, &h.pd, &ps); }
        catch (const TranscriptMismatch &) { h.pd.verdict = ZP_VERDICT_TRANSCRIPT; }
        if (h.rc == ZP_ERR_UNSUPPORTED) { h.rc = ZP_OK; h.pd.verdict = ZP_VERDICT_PARAMS; }      // an inner header that names the BN128 hash
        if (h.rc != ZP_OK) { nj->rc = h.rc; return; }
        if (h.pd.verdict != ZP_VERDICT_ACCEPT) return;      // the stream position means nothing behind a header that failed
    }
    if (ps.pos != ps.n) { nj->post_verdict = ZP_VERDICT_TRANSCRIPT; return; }
    // roots, then the leaf index of every (slot, proof, tree): the index of query slot mod n_queries, cut to the tree's depth
    const int logm = S.vp.logn + S.vp.logb;
    std::vector<int> depths = {logm};
    if (S.pg.W2) depths.push_back(logm);
    depths.push_back(logm);
    for (auto &lf : sched) depths.push_back(lf.first - lf.second);
    std::vector<u64> want;
    want.reserve(n_merkle > n_tail ? n_merkle : n_tail);
    for (const HeaderJob &h : nj->hdr) {
        want.insert(want.end(), h.raw.root[0].begin(), h.raw.root[0].end());
        if (S.pg.W2) want.insert(want.end(), h.raw.root[1].begin(), h.raw.root[1].end());
        want.insert(want.end(), h.raw.root[2].begin(), h.raw.root[2].end());
        want.insert(want.end(), h.raw.fri_roots.begin(), h.raw.fri_roots.end());
    }
    for (size_t g = 0; g < n_slots; g++)
        for (const HeaderJob &h : nj->hdr)
            for (int d : depths) want.push_back(h.pd.qidx[g % nq] & (((u64)1 << d) - 1));
    if (want.size() != n_merkle || memcmp(want.data(), pubs.data(), 8 * n_merkle) != 0) { nj->post_verdict = ZP_VERDICT_PUBLICS; return; }
    want.clear();
    for (const HeaderJob &h : nj->hdr) arithmetic_publics(h.pd, S.pg, S.vp, &want);
    const u64 mask = ((u64)1 << final_log) - 1;
    for (size_t g = 0; g < n_slots; g++)
        for (const HeaderJob &h : nj->hdr)
            for (int c = 0; c < 3; c++) want.push_back(h.raw.final_l[c][h.pd.qidx[g % nq] & mask]);
    if (want.size() != n_tail || memcmp(want.data(), pubs.data() + pubs.size() - n_tail, 8 * n_tail) != 0) nj->post_verdict = ZP_VERDICT_PUBLICS;
}

int32_t aggregate_verify_impl(zp_ctx *ctx, const zp_agg_statement *stmts, int32_t n_stmts, const char *const *texts, const size_t *lens, int32_t n_texts, uint32_t flags,
                              int32_t threads, int32_t *verdicts, int32_t *where) {
    if (!stmts || n_stmts < 1 || n_stmts > 64 || !texts || !lens || !verdicts || n_texts < 1 || n_texts > (1 << 20) || (flags & ~(uint32_t)ZP_VERIFY_HEADER_ONLY)) return ZP_ERR_ARG;
    for (int32_t i = 0; i < n_texts; i++)
        if (!texts[i]) return ZP_ERR_ARG;
    // the table of statements
    std::vector<AggStmt> st((size_t)n_stmts);
    int leaves = 0;
    for (int32_t i = 0; i < n_stmts; i++) {
        const zp_agg_statement &a = stmts[i];
        AggStmt &S = st[i];
        S.vp = {a.logn, a.logb, a.fri_logf, a.fri_final_log, a.n_queries, a.pow_bits, flags, 1, ctx ? ctx->root32 : ZP_ROOT32_DEFAULT, ctx ? ctx->coset_shift : ZP_SHIFT_DEFAULT, nullptr};
        if (!a.h_program || !params_in_range(S.vp) || !program_info(a.h_program, a.program_words, &S.pg)) return ZP_ERR_ARG;
        S.leaf = a.shape_json == nullptr;
        leaves += S.leaf;
        if (!S.leaf) {
            Cur c{a.shape_json, a.shape_json + strlen(a.shape_json)};
            bool in_range = false;
            if (!parse_shape(c, S.shape, &in_range) || !in_range) return ZP_ERR_ARG;
            c.ws();
            if (c.p != c.end || a.n_slots < 1 || a.n_slots > (1 << 20)) return ZP_ERR_ARG;
            S.n_slots = (size_t)a.n_slots;
        }
    }
    if (leaves > 1) return ZP_ERR_ARG;
    const HostPoseidon H = {ctx ? ctx->h_rc : (const u64 *)ZP_POSEIDON_DEFAULT_RC, ctx ? ctx->h_mds : (const u64 *)ZP_POSEIDON_DEFAULT_MDS};
    const bool header_only = (flags & ZP_VERIFY_HEADER_ONLY) != 0;

    // 1. grammar and structure of every text
    std::vector<TextJob> tj((size_t)n_texts);
    struct Unit { TextJob *t; NodeJob *n; };   // n = NULL: the outer STARK's header
    std::vector<Unit> units;
    for (int32_t i = 0; i < n_texts; i++) {
        TextJob &t = tj[i];
        Cur c{texts[i], texts[i] + lens[i]};
        const bool ok = parse_node(c, &t.top, 1);
        c.ws();
        if (!ok || !c.ok || c.p != c.end || !t.top.has_stark || !t.top.has_inner) { t.verdict = ZP_VERDICT_MALFORMED; continue; }
        if (t.top.has_shape && !t.top.shape_ok) { t.verdict = ZP_VERDICT_MALFORMED; continue; }
        if (too_deep(t.top)) { t.verdict = ZP_VERDICT_TREE; continue; }
        if (t.top.has_shape) t.top_stmt = find_stmt(st, t.top.shape);
        else for (size_t k = 0; k < st.size() && t.top_stmt < 0; k++) if (!st[k].leaf) t.top_stmt = (int)k;
        if (t.top_stmt < 0) { t.verdict = ZP_VERDICT_PARAMS; continue; }
        t.outer.text = t.top.stark; t.outer.stmt = t.top_stmt;
        if (!parse_header(t.top.stark.p, t.top.stark.n, false, &t.outer.raw)) { t.verdict = ZP_VERDICT_MALFORMED; continue; }
        units.push_back({&t, nullptr});
        plan_node(&t, t.top, &t.outer.raw.pubs, st, true);
        for (NodeJob *n : t.nodes)
            if (n->verdict == ZP_VERDICT_ACCEPT) units.push_back({&t, n});
    }
    // 2. every header phase (a transcript is a serial chain; nodes and texts are independent).  The transcripts of the outer STARKs of all texts are
    // one chain launch where they go to the device; inner headers are READ off their vouching public inputs either way
    DeviceTranscripts dt;
    std::vector<size_t> outer_slot(units.size(), 0);
    if (chains_on_device(ctx, false)) {
        std::vector<PlanItem> items;
        for (size_t u = 0; u < units.size(); u++)
            if (!units[u].n) {
                const TextJob &t = *units[u].t;
                outer_slot[u] = items.size();
                items.push_back({t.outer.text.p, t.outer.text.n, &st[t.top_stmt].pg, &st[t.top_stmt].vp});
            }
        ZP_TRY(dt.run(ctx, false, items));
    }
    spread(units.size(), threads, [&](size_t u) {
        TextJob &t = *units[u].t;
        int32_t *rc = units[u].n ? &units[u].n->rc : &t.outer.rc;
        try {
            if (units[u].n) { run_node(units[u].n, st, H); return; }
            t.outer.pd.defer_identity = true;
            const AggStmt &S = st[t.top_stmt];
            *rc = dt.on ? dt.header(outer_slot[u], t.outer.text.p, t.outer.text.n, S.pg, S.vp, H, &t.outer.pd) : header_phase(t.outer.text.p, t.outer.text.n, S.pg, S.vp, H, &t.outer.pd);
        } catch (const std::bad_alloc &) { *rc = ZP_ERR_NOMEM; }
        catch (...) { *rc = ZP_ERR_INTERNAL; }
    });
    for (const Unit &u : units) {
        const int32_t rc = u.n ? u.n->rc : u.t->outer.rc;
        if (rc != ZP_OK) {
            if (ctx) ctx->err = rc == ZP_ERR_UNSUPPORTED ? "an outer STARK in BN128-hash mode (or a build without the openings parser)" : "a program blob could not be evaluated at a proof's point";
            return rc;
        }
    }
    // 3. the fixed columns of every pending identity, one call per statement; then the constraint programs
    std::vector<std::vector<HeaderJob *>> by_stmt(st.size());
    for (const Unit &u : units) {
        if (!u.n) { if (u.t->outer.pd.id_pending) by_stmt[u.t->top_stmt].push_back(&u.t->outer); continue; }
        for (HeaderJob &h : u.n->hdr)
            if (h.pd.id_pending) by_stmt[h.stmt].push_back(&h);
    }
    for (size_t k = 0; k < st.size(); k++) {
        std::vector<HeaderJob *> &jobs = by_stmt[k];
        if (jobs.empty()) continue;
        const AggStmt &S = st[k];
        const size_t n = jobs.size(), npc = S.pg.n_pub + S.pg.n_chal, n_fixed = S.pg.n_fixed;
        std::vector<u64> pc(n * npc + 1), zeta(n * 3), fixed(n * n_fixed * 3);
        std::vector<uint8_t> on_domain(n);
        for (size_t i = 0; i < n; i++) {
            if (npc) memcpy(&pc[i * npc], jobs[i]->pd.id_pubchal.data(), 8 * npc);
            memcpy(&zeta[3 * i], jobs[i]->pd.zeta.c, 24);
        }
        const int32_t rc = zp_program_fixed_eval_ext_batch(ctx, S.pg.words, S.pg.n_words, (const uint64_t *)pc.data(), (int32_t)npc, S.vp.logn, S.vp.root32, (const uint64_t *)zeta.data(),
                                                           (int32_t)n, (uint64_t *)fixed.data(), (int32_t)n_fixed, on_domain.data(), threads);
        if (rc != ZP_OK) { if (ctx && ctx->err.empty()) ctx->err = "a program blob could not be evaluated at a proof's point"; return rc; }
        std::vector<int32_t> rcs(n, ZP_OK);
        spread(n, threads, [&](size_t i) {
            HeaderJob &h = *jobs[i];
            if (on_domain[i]) { h.id_verdict = ZP_VERDICT_IDENTITY; return; }
            try { rcs[i] = identity_at_zeta(S.pg, S.vp, h.pd.id_pubchal, h.pd.id_alpha, h.pd.zeta, h.pd.ev_z, h.pd.ev_zw, (const uint64_t *)&fixed[i * n_fixed * 3], 1, &h.id_verdict); }
            catch (...) { rcs[i] = ZP_ERR_NOMEM; }
        });
        for (int32_t r : rcs)
            if (r != ZP_OK) return r;
    }
    // 4. the query phase of the outer STARKs that got this far, statement by statement (one launch each on a ctx)
    for (size_t k = 0; k < st.size() && !header_only; k++) {
        std::vector<TextJob *> live;
        for (TextJob &t : tj)
            if (t.verdict == ZP_VERDICT_ACCEPT && t.top_stmt == (int)k && t.outer.id_verdict == ZP_VERDICT_ACCEPT && t.outer.pd.queries_live) live.push_back(&t);
        if (live.empty()) continue;
        std::vector<Pending> pend(live.size());
        for (size_t i = 0; i < live.size(); i++) pend[i] = std::move(live[i]->outer.pd);
        VerifyParams vp = st[k].vp;
        vp.threads = threads;
        const int32_t rc = queries_phase(ctx, vp, H, pend, st[k].pg.n_s2 != 0);
        for (size_t i = 0; i < live.size(); i++) live[i]->outer.pd = std::move(pend[i]);
        if (rc != ZP_OK) return rc;
    }
    // 5. the first failing check in the documented order
    for (int32_t i = 0; i < n_texts; i++) {
        TextJob &t = tj[i];
        auto header_verdict = [](const HeaderJob &h) { return h.pd.id_pending && h.id_verdict != ZP_VERDICT_ACCEPT ? h.id_verdict : h.pd.verdict; };
        if (t.verdict == ZP_VERDICT_ACCEPT) t.verdict = header_verdict(t.outer);
        for (size_t k = 0; k < t.nodes.size() && t.verdict == ZP_VERDICT_ACCEPT; k++) {
            const NodeJob &n = *t.nodes[k];
            int v = n.verdict;
            for (size_t j = 0; j < n.hdr.size() && v == ZP_VERDICT_ACCEPT; j++) v = header_verdict(n.hdr[j]);
            if (v == ZP_VERDICT_ACCEPT) v = n.post_verdict;
            if (v != ZP_VERDICT_ACCEPT) { t.verdict = v; t.where = (int)k; }
        }
        verdicts[i] = t.verdict;
    }
    if (where) *where = tj[0].where;
    return ZP_OK;
}

}  // namespace

extern "C" {

int32_t zp_stark_verify(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const char *proof_json, size_t proof_len, int32_t logn, int32_t logb, int32_t fri_logf,
                        int32_t fri_final_log, int32_t n_queries, int32_t pow_bits, uint32_t flags, int32_t threads, int32_t *verdict, int32_t *where, uint64_t *h_indices) {
    if (!verdict || !where) return ZP_ERR_ARG;
    *verdict = ZP_VERDICT_MALFORMED;
    *where = -1;
    const VerifyParams vp = {logn, logb, fri_logf, fri_final_log, n_queries, pow_bits, flags, threads, 0, 0, nullptr};
    return verify_guarded(ctx, [&] { return verify_batch_impl(ctx, h_program, program_words, &proof_json, &proof_len, 1, vp, verdict, where, h_indices); });
}

int32_t zp_stark_verify_batch(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const char *const *proofs, const size_t *lens, int32_t n_proofs, int32_t logn,
                              int32_t logb, int32_t fri_logf, int32_t fri_final_log, int32_t n_queries, int32_t pow_bits, uint32_t flags, int32_t threads, int32_t *verdicts) {
    const VerifyParams vp = {logn, logb, fri_logf, fri_final_log, n_queries, pow_bits, flags, threads, 0, 0, nullptr};
    return verify_guarded(ctx, [&] { return verify_batch_impl(ctx, h_program, program_words, proofs, lens, n_proofs, vp, verdicts, nullptr, nullptr); });
}

int32_t zp_stark_verify_bn128(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const char *proof_json, size_t proof_len, int32_t logn, int32_t logb,
                              int32_t fri_logf, int32_t fri_final_log, int32_t n_queries, int32_t rp, const uint64_t *h_rc, const uint64_t *h_mds, uint32_t flags,
                              int32_t threads, int32_t *verdict, int32_t *where, uint64_t *h_indices) {
    if (!verdict || !where) return ZP_ERR_ARG;
    *verdict = ZP_VERDICT_MALFORMED;
    *where = -1;
    return verify_guarded(ctx, [&] {
        HostPoseidon254 H254;
        ZP_TRY(tables254(ctx, rp, h_rc, h_mds, &H254));
        const VerifyParams vp = {logn, logb, fri_logf, fri_final_log, n_queries, 0, flags, threads, 0, 0, &H254};
        return verify_batch_impl(ctx, h_program, program_words, &proof_json, &proof_len, 1, vp, verdict, where, h_indices);
    });
}

int32_t zp_stark_verify_batch_bn128(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const char *const *proofs, const size_t *lens, int32_t n_proofs,
                                    int32_t logn, int32_t logb, int32_t fri_logf, int32_t fri_final_log, int32_t n_queries, int32_t rp, const uint64_t *h_rc,
                                    const uint64_t *h_mds, uint32_t flags, int32_t threads, int32_t *verdicts) {
    return verify_guarded(ctx, [&] {
        HostPoseidon254 H254;
        ZP_TRY(tables254(ctx, rp, h_rc, h_mds, &H254));
        const VerifyParams vp = {logn, logb, fri_logf, fri_final_log, n_queries, 0, flags, threads, 0, 0, &H254};
        return verify_batch_impl(ctx, h_program, program_words, proofs, lens, n_proofs, vp, verdicts, nullptr, nullptr);
    });
}

// The chain primitive of the BN128-mode transcripts on its own: chain c walks the steps [h_first[c], h_first[c + 1]) from the zero state; a step
// overwrites elements 1..16 with its block when h_absorb says so, then permutes; h_rates receives the rate after every step.  With a ctx: the
// installed tables, all chains in one launch (csrc/poseidon_bn254.hip: sponge_chains254_kernel); ctx = NULL: the caller's tables, HostPoseidon254
int32_t zp_poseidon_bn254_chains(zp_ctx *ctx, const uint64_t *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int32_t nchains, int32_t rp, const uint64_t *h_rc,
                                 const uint64_t *h_mds, uint64_t *h_rates) {
    return verify_guarded(ctx, [&]() -> int32_t {
        auto bad = [&](const char *msg) { if (ctx) ctx->err = std::string("bad argument: ") + msg; return ZP_ERR_ARG; };
        if (nchains < 0) return bad("nchains < 0");
        if (nchains > 0 && !h_first) return bad("null h_first");
        size_t nsteps = 0;
        if (nchains > 0) {
            if (h_first[0] != 0) return bad("h_first must start at 0");
            for (int32_t c = 0; c < nchains; c++)
                if (h_first[c + 1] < h_first[c]) return bad("h_first must be non-decreasing");
            nsteps = h_first[nchains];
        }
        if (nsteps >= ((size_t)1 << 24)) return bad("too many steps");
        if (nsteps && (!h_blocks || !h_absorb || !h_rates)) return bad("null pointer");
        for (size_t i = 0; i < nsteps * 16; i++)
            if (!fr_is_canonical_u64((const u64 *)h_blocks + 4 * i)) return bad("block element not reduced mod r");
        HostPoseidon254 H254;
        ZP_TRY(tables254(ctx, rp, h_rc, h_mds, &H254));
        if (!nsteps) return ZP_OK;
        if (ctx) {
            if (!zpi_poseidon254_chains_host) { ctx->err = "this build has no device side"; return ZP_ERR_UNSUPPORTED; }
            return zpi_poseidon254_chains_host(ctx, (const u64 *)h_blocks, h_absorb, h_first, nchains, (u64 *)h_rates);
        }
        for (int32_t c = 0; c < nchains; c++) {
            HostSponge254 sp(H254);
            for (size_t s = h_first[c]; s < h_first[c + 1]; s++) {
                sp.step(h_absorb[s] != 0, (const u64 *)h_blocks + 64 * s);
                sp.rate((u64 *)h_rates + 64 * s);
            }
        }
        return ZP_OK;
    });
}

// since zp_create: chain launches; chain steps run on the device; public-input commitments made on the device; texts that fell back to the host sponge
int32_t zp_verify_counters(zp_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return ZP_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = ctx->verify_counters[i];
    return ZP_OK;
}

int32_t zp_aggregate_verify(zp_ctx *ctx, const zp_agg_statement *stmts, int32_t n_stmts, const char *text, size_t len, uint32_t flags, int32_t threads, int32_t *verdict,
                            int32_t *where) {
    if (!verdict || !where) return ZP_ERR_ARG;
    *verdict = ZP_VERDICT_MALFORMED;
    *where = -1;
    return verify_guarded(ctx, [&] { return aggregate_verify_impl(ctx, stmts, n_stmts, &text, &len, 1, flags, threads, verdict, where); });
}

int32_t zp_aggregate_verify_batch(zp_ctx *ctx, const zp_agg_statement *stmts, int32_t n_stmts, const char *const *texts, const size_t *lens, int32_t n_texts, uint32_t flags,
                                  int32_t threads, int32_t *verdicts) {
    return verify_guarded(ctx, [&] { return aggregate_verify_impl(ctx, stmts, n_stmts, texts, lens, n_texts, flags, threads, verdicts, nullptr); });
}

}  // extern "C"
