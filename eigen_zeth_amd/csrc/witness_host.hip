// zp_stark_check_witness: does a trace satisfy a constraint program, and if not, which constraint at which row -- the check BEFORE a proof
// (GenChunkProof, proto/prover/v1/prover.proto:56-66: a client that hands in a witness no verifier would accept gets a reason instead of a
// well-formed, worthless proof).  No reference counterpart (the prover behind src/prover/provider.rs:358-377 is external); the checker's own
// statement of the same is oracle/air_program.py: Program.evaluate_base per row.
// This file is HOST code only and builds on its own as plain C++ (tests/test_witness_check_fuzz.py links it with csrc/verify.hip under the host
// sanitizers): the entry point, every refusal, the derived challenge, and the whole check for ctx = NULL.  With a ctx the validated arguments go
// to csrc/witness_check.hip (a weak reference: absent in the sanitizer build, where only ctx = NULL is served).
// The blob is read and walked by air_program.hpp (zpi_program_read with ZPG_WITNESS, zpi_program_walk), the field code is gl.hpp's: no decoder of its own.
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "sha256.hpp"

extern int32_t zpi_witness_check_device(zp_ctx *ctx, const ZpProgram &pg, const std::vector<u64> &pubchal, const u64 *d_trace, int logn, uint64_t *h_report,
                                        uint64_t *h_counts, uint64_t *h_first_row) __attribute__((weak));

namespace {

constexpr u64 NONE = ~0ULL;

// the stage-2 columns of a trace from their definitions (include/zeth_prover.h: zp_grand_product, zp_logup_columns), one inversion per row -- the
// device primitives divide row by row too, so a vanishing denominator (1/0 = 0 in e3_inv) gives the same words on both paths
void stage2_columns(const ZpProgram &pg, const u64 *trace, size_t N, const e3 &g, u64 *s2) {
    size_t at = 0;
    for (size_t k = 0; k < pg.n_s2; k++) {
        const u64 *st = pg.stage2 + 4 * k;
        const u64 *a = trace + st[1] * N, *b = trace + st[2] * N, *m = trace + st[3] * N;
        u64 *o = s2 + at * N;
        if (st[0] == 1) {
            e3 z = e3_make(1, 0, 0);
            for (size_t i = 0; i < N; i++) {
                for (int c = 0; c < 3; c++) o[c * N + i] = z.c[c];
                const e3 num = e3_make(gl_add(a[i], g.c[0]), g.c[1], g.c[2]), den = e3_make(gl_add(b[i], g.c[0]), g.c[1], g.c[2]);
                z = e3_mul(z, e3_mul(num, e3_inv(den)));
            }
            at += 3;
        } else {
            e3 s = e3_make(0, 0, 0);
            for (size_t i = 0; i < N; i++) {
                const e3 h1 = e3_inv(e3_make(gl_add(a[i], g.c[0]), g.c[1], g.c[2]));
                const e3 h2 = e3_scale(e3_inv(e3_make(gl_add(b[i], g.c[0]), g.c[1], g.c[2])), m[i]);
                for (int c = 0; c < 3; c++) {
                    o[c * N + i] = h1.c[c];
                    o[(3 + c) * N + i] = h2.c[c];
                    o[(6 + c) * N + i] = s.c[c];
                }
                s = e3_add(s, e3_sub(h1, h2));
            }
            at += 9;
        }
    }
}

// the environment of zpi_program_walk for one trace row over the base field
struct HostEnv {
    typedef u64 value;
    static u64 add(u64 a, u64 b) { return gl_add(a, b); }
    static u64 sub(u64 a, u64 b) { return gl_sub(a, b); }
    static u64 mul(u64 a, u64 b) { return gl_mul(a, b); }
    const ZpProgram *pg;
    const u64 *trace, *s2, *pubchal;
    const std::vector<std::vector<u64>> *periods;
    size_t N, r, rn;
    u64 xml;
    u64 *counts, *first;       // of the rows walked so far: counts[k] = violated rows of constraint k, first[k] = the smallest of them
    u64 file[32];
    u64 &slot(int i) { return file[i]; }
    u64 column(size_t idx, size_t row) const { return idx < pg->W ? trace[idx * N + row] : s2[(idx - pg->W) * N + row]; }
    u64 load(int kind, int idx) const {
        switch (kind) {
            case ZPK_SLOT: return file[idx];
            case ZPK_COL: return column(idx, r);
            case ZPK_NEXT: return column(idx, rn);
            case ZPK_FIXED: {
                if (idx < 2) return idx == 0 ? r == 0 : r == N - 1;
                const std::vector<u64> &p = (*periods)[idx - 2];
                return p[r & (p.size() - 1)];
            }
            case ZPK_PUB: return pubchal[idx];
            case ZPK_CONST: return pg->consts[idx];
            default: return xml;
        }
    }
    void out(int k, u64 v) {
        if (v == 0) return;
        counts[k]++;
        if (first[k] == NONE) first[k] = r;
    }
};

// rows [r0, r1) in ascending order
void check_rows(HostEnv h, u64 wN, u64 wlast, size_t r0, size_t r1, u64 *counts, u64 *first) {
    h.counts = counts; h.first = first;
    memset(h.file, 0, sizeof h.file);
    u64 x = gl_pow(wN, (u64)r0);
    for (size_t r = r0; r < r1; r++, x = gl_mul(x, wN)) {
        h.r = r; h.rn = (r + 1) & (h.N - 1); h.xml = gl_sub(x, wlast);
        zpi_program_walk(h.pg->ins, (int)h.pg->n_instr, h);
    }
}

// the t-th of T near-equal ranges of n items
inline void share(size_t n, unsigned T, unsigned t, size_t *a, size_t *b) { *a = n * t / T; *b = n * (t + 1) / T; }

int32_t check_host(const ZpProgram &pg, const std::vector<u64> &pubchal, const u64 *trace, int logn, int threads, uint64_t *h_report, uint64_t *h_counts,
                   uint64_t *h_first_row) {
    const size_t N = (size_t)1 << logn, K = pg.K, words = pg.W * N;
    const unsigned T = zpi_host_threads(threads);
    // (1) every word of the trace, read or not by an instruction, against p
    std::vector<u64> bad_n(T, 0), bad_at(T, NONE);
    {
        const unsigned Tc = words < 4096 ? 1 : T;
        zpi_over_threads(Tc, [&](unsigned t) noexcept {
            size_t a, b;
            share(words, Tc, t, &a, &b);
            for (size_t i = a; i < b; i++)
                if (trace[i] >= GL_P) { bad_n[t]++; if (bad_at[t] == NONE) bad_at[t] = i; }
        });
    }
    u64 n_bad = 0, at_bad = NONE;
    for (unsigned t = 0; t < T; t++) { n_bad += bad_n[t]; if (bad_at[t] < at_bad) at_bad = bad_at[t]; }
    u64 rep[8] = {ZP_WITNESS_SATISFIED, NONE, NONE, 0, 0, n_bad, NONE, NONE};
    std::vector<u64> counts(K, 0), first(K, NONE);
    if (n_bad) {
        rep[0] = ZP_WITNESS_NONCANONICAL;
        rep[6] = at_bad / N;
        rep[7] = at_bad % N;
    } else {
        // (2) the stage-2 columns and one period of every sparse fixed column
        std::vector<u64> s2(pg.W2 * N);
        if (pg.n_s2) stage2_columns(pg, trace, N, e3_make(pubchal[pg.n_pub], pubchal[pg.n_pub + 1], pubchal[pg.n_pub + 2]), s2.data());
        std::vector<std::vector<u64>> periods(pg.fxc.size());
        for (size_t k = 0; k < pg.fxc.size(); k++) {
            const ZpFixedCol &fc = pg.fxc[k];
            periods[k].assign((size_t)1 << fc.lp, 0);
            for (size_t e = 0; e < fc.n_entries; e++) {
                const ZpFixedEntry en = zpi_fixed_entry(pg.words, fc, e);
                periods[k][en.pos] = en.is_pub ? pubchal[en.value] : en.value;
            }
        }
        // (3) rows over threads, per-thread counts merged at the end
        const unsigned Tr = N < 64 ? 1 : (N / 16 < T ? (unsigned)(N / 16) : T);
        std::vector<u64> tc((size_t)Tr * K, 0), tf((size_t)Tr * K, NONE);
        HostEnv h{};
        h.pg = &pg; h.trace = trace; h.s2 = s2.data(); h.pubchal = pubchal.data(); h.periods = &periods; h.N = N;
        const u64 wN = gl_root(ZP_ROOT32_DEFAULT, logn), wlast = gl_inv(wN);
        zpi_over_threads(Tr, [&](unsigned t) noexcept {
            size_t a, b;
            share(N, Tr, t, &a, &b);
            check_rows(h, wN, wlast, a, b, &tc[(size_t)t * K], &tf[(size_t)t * K]);
        });
        for (unsigned t = 0; t < Tr; t++)
            for (size_t k = 0; k < K; k++) {
                counts[k] += tc[(size_t)t * K + k];
                if (tf[(size_t)t * K + k] < first[k]) first[k] = tf[(size_t)t * K + k];
            }
        for (size_t k = 0; k < K; k++) {
            rep[3] += counts[k];
            rep[4] += counts[k] != 0;
            if (first[k] < rep[1]) { rep[1] = first[k]; rep[2] = k; }       // ascending k: the smallest index on the smallest row
        }
        if (rep[3]) rep[0] = ZP_WITNESS_VIOLATED;
    }
    memcpy(h_report, rep, sizeof rep);
    if (h_counts) memcpy(h_counts, counts.data(), K * 8);
    if (h_first_row) memcpy(h_first_row, first.data(), K * 8);
    return ZP_OK;
}

}  // namespace

// What zp_stark_check_witness and zp_stark_check_witness_sharded (csrc/witness_sharded.hip) require of their arguments, and what they derive from
// them: the parsed program and [publics | challenge (given, or derived from the program) | 0].  The trace behind `trace` holds the columns of `rank`
// among `world` (zpi_shard_range; world = 1: all of them) and may be NULL when that is none.  Returns NULL, or why the call is refused.
const char *zpi_witness_args(const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words, int world, int rank,
                             const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, const uint64_t *h_chal3, const uint64_t *h_report, const uint64_t *h_counts,
                             const uint64_t *h_first_row, int32_t n_constraints, ZpProgram *pgp, std::vector<u64> *pubchal) {
    const char *why = "";
    ZpProgram &pg = *pgp;
    if (!zpi_program_read(h_program, program_words, ZPG_WITNESS, &pg, &why)) return why;
    size_t first, cols;
    zpi_shard_range(pg.W, world, rank, &first, &cols);
    if ((!trace && cols) || !h_report) return "null pointer";
    if (logn < 1 || logn > 32) return "logn out of range";
    if (trace_words != cols << logn) return world == 1 ? "trace_words must be W * 2^logn" : "trace_words must be (this rank's columns) * 2^logn";
    if (n_pubs < 0 || (size_t)n_pubs != pg.n_pub || (n_pubs && !h_pubs)) return "number of public inputs does not match the program";
    for (int i = 0; i < n_pubs; i++)
        if (h_pubs[i] >= GL_P) return "public input not canonical";
    for (const ZpFixedCol &fc : pg.fxc)
        if (fc.lp > logn) return "fixed column longer than the trace";
    if ((h_counts || h_first_row) && (n_constraints < 0 || (size_t)n_constraints != pg.K)) return "n_constraints is not the program's";
    pubchal->assign(h_pubs, h_pubs + n_pubs);
    if (pg.n_s2) {
        u64 g[3];
        if (h_chal3) {
            for (int c = 0; c < 3; c++) {
                if (h_chal3[c] >= GL_P) return "challenge not canonical";
                g[c] = h_chal3[c];
            }
        } else {                      // derived from the statement: finds mistakes, binds nobody (the header says so)
            uint8_t dg[32];
            Sha256::digest((const uint8_t *)h_program, program_words * 8, dg);
            for (int i = 0; i < 3; i++) { u64 x = 0; for (int b = 7; b >= 0; b--) x = (x << 8) | dg[8 * i + b]; g[i] = x % GL_P; }
            if (g[1] == 0 && g[2] == 0) g[1] = 1;       // outside the base field: value + g is never 0
        }
        pubchal->insert(pubchal->end(), g, g + 3);
    }
    pubchal->push_back(0);            // never empty: both paths take its address
    return nullptr;
}

extern "C" int32_t zp_stark_check_witness(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words,
                                          const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, const uint64_t *h_chal3, uint64_t *h_report,
                                          uint64_t *h_counts, uint64_t *h_first_row, int32_t n_constraints, int32_t threads) {
    try {
        ZpProgram pg;
        std::vector<u64> pubchal;
        if (const char *why = zpi_witness_args(h_program, program_words, trace, trace_words, 1, 0, h_pubs, n_pubs, logn, h_chal3, h_report, h_counts, h_first_row,
                                               n_constraints, &pg, &pubchal)) {
            if (ctx) {
                try { ctx->err = std::string("bad argument: ") + why; } catch (...) {}
            }
            return ZP_ERR_ARG;
        }
        if (ctx) {
            if (!zpi_witness_check_device) { ctx->err = "this build has no device witness check"; return ZP_ERR_UNSUPPORTED; }
            return zpi_witness_check_device(ctx, pg, pubchal, (const u64 *)trace, logn, h_report, h_counts, h_first_row);
        }
        return check_host(pg, pubchal, (const u64 *)trace, logn, threads, h_report, h_counts, h_first_row);
    } catch (const std::bad_alloc &) {
        return ZP_ERR_NOMEM;
    } catch (...) {
        return ZP_ERR_INTERNAL;
    }
}
