// zp_stark_diagnose_stage2: WHICH cell breaks a permutation or a lookup.  zp_stark_check_witness (csrc/witness_host.hip) reports a broken stage-2
// argument at row N - 1, where the running product or sum fails to close; a running product cannot say more.  What can is a comparison of multisets
// (include/zeth_prover.h): per value v, lhs(v) = occurrences in column a against rhs(v) = occurrences in b (permutation) or the sum of m over the
// rows with t = v, mod p (lookup).  No reference counterpart (the prover behind src/prover/provider.rs:358-377 is external).
// This file is HOST code only and builds on its own as plain C++ (tests/test_stage2_diag_fuzz.py links it alone under the host sanitizers): the
// entry point, every refusal, the records of a non-canonical trace, and the whole computation for ctx = NULL.  With a ctx the validated arguments
// go to csrc/stage2_diag.hip (a weak reference: absent in the sanitizer build, where only ctx = NULL is served).
// The blob is read by air_program.hpp (zpi_program_read with ZPG_WITNESS, the group zp_stark_check_witness asks for): no decoder of its own.
#include <cstring>
#include <exception>
#include <thread>
#include <unordered_map>
#include <vector>

#include "ctx.hpp"

extern int32_t zpi_stage2_diag_device(zp_ctx *ctx, const ZpProgram &pg, const u64 *d_trace, int logn, uint64_t *h_diag) __attribute__((weak));

namespace {

constexpr u64 NONE = ~0ULL;

struct Tally { u64 lhs = 0; unsigned __int128 rhs = 0; u64 first_a = NONE, first_b = NONE; };
// which of T shares owns value v: any function of v alone will do (the records do not depend on it)
inline unsigned owner(u64 v, unsigned T) { return (unsigned)(((v ^ (v >> 32)) * 0x9E3779B97F4A7C15ULL >> 33) % T); }

struct Share {
    std::unordered_map<u64, Tally> map;
    u64 unbalanced = 0, rows_a = 0, r_a = NONE, r_b = NONE;
    bool failed = false;
};

// one argument: every thread walks both columns and tallies the values it owns, then judges them; the shares are merged in thread order
int32_t diagnose_argument(const u64 *st, const u64 *trace, size_t N, unsigned T, u64 *rec) {
    const u64 *a = trace + st[1] * N, *b = trace + st[2] * N, *m = st[0] == ZPS2_LOGUP ? trace + st[3] * N : nullptr;
    std::vector<Share> shares(T);
    zpi_over_threads(T, [&](unsigned t) noexcept {
        Share &s = shares[t];
        try {
            for (size_t r = 0; r < N; r++) {
                if (T == 1 || owner(a[r], T) == t) {
                    Tally &y = s.map[a[r]];
                    y.lhs++;
                    if (y.first_a == NONE) y.first_a = r;
                }
                if (T == 1 || owner(b[r], T) == t) {
                    Tally &y = s.map[b[r]];
                    y.rhs += m ? m[r] : 1;
                    if (y.first_b == NONE) y.first_b = r;
                }
            }
            for (const auto &kv : s.map) {
                const Tally &y = kv.second;
                if (y.lhs == (u64)(y.rhs % GL_P)) continue;
                s.unbalanced++;
                s.rows_a += y.lhs;
                if (y.first_a < s.r_a) s.r_a = y.first_a;
                if (y.first_b < s.r_b) s.r_b = y.first_b;
            }
        } catch (...) { s.failed = true; }
    });
    u64 out[ZP_S2_WORDS] = {ZP_S2_HOLDS, st[0], 0, NONE, NONE, 0, 0, NONE, NONE, 0, 0, 0};
    for (const Share &s : shares) {
        if (s.failed) return ZP_ERR_NOMEM;
        out[2] += s.unbalanced;
        out[11] += s.rows_a;
        if (s.r_a < out[3]) out[3] = s.r_a;
        if (s.r_b < out[7]) out[7] = s.r_b;
    }
    if (out[2]) out[0] = ZP_S2_FAILS;
    for (int side = 0; side < 2; side++) {
        const u64 row = out[side ? 7 : 3];
        if (row == NONE) continue;
        const u64 v = (side ? b : a)[row];
        const Tally &y = shares[T == 1 ? 0 : owner(v, T)].map.at(v);
        u64 *o = out + (side ? 8 : 4);
        o[0] = v; o[1] = y.lhs; o[2] = (u64)(y.rhs % GL_P);
    }
    memcpy(rec, out, sizeof out);
    return ZP_OK;
}

int32_t diagnose_host(const ZpProgram &pg, const u64 *trace, int logn, int threads, uint64_t *h_diag) {
    const size_t N = (size_t)1 << logn, words = pg.W * N;
    const unsigned T = N < 4096 ? 1 : zpi_host_threads(threads);
    // every word of the trace, read or not by an argument, against p (the witness check's first pass)
    std::vector<u64> bad(T, 0);
    zpi_over_threads(T, [&](unsigned t) noexcept {
        for (size_t i = words * t / T, e = words * (t + 1) / T; i < e; i++) bad[t] |= trace[i] >= GL_P;
    });
    std::vector<u64> out(pg.n_s2 * ZP_S2_WORDS);
    bool any = false;
    for (unsigned t = 0; t < T; t++) any |= bad[t] != 0;
    if (any) zpi_stage2_diag_noncanonical(pg, (uint64_t *)out.data());
    else
        for (size_t j = 0; j < pg.n_s2; j++) ZP_TRY(diagnose_argument(pg.stage2 + 4 * j, trace, N, T, &out[j * ZP_S2_WORDS]));
    memcpy(h_diag, out.data(), out.size() * 8);
    return ZP_OK;
}

}  // namespace

// the records of a trace with words >= p: nothing is compared (the empty key of the device table, ~0, is told from a value only among canonical words)
void zpi_stage2_diag_noncanonical(const ZpProgram &pg, uint64_t *h_diag) {
    for (size_t j = 0; j < pg.n_s2; j++) {
        const u64 rec[ZP_S2_WORDS] = {ZP_S2_NONCANONICAL, pg.stage2[4 * j], 0, NONE, NONE, 0, 0, NONE, NONE, 0, 0, 0};
        memcpy(h_diag + j * ZP_S2_WORDS, rec, sizeof rec);
    }
}

extern "C" int32_t zp_stark_diagnose_stage2(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words, int32_t logn,
                                            uint64_t *h_diag, int32_t n_stage2, int32_t threads) {
    try {
        ZpProgram pg;
        const char *why = "";
        if (zpi_program_read(h_program, program_words, ZPG_WITNESS, &pg, &why)) {
            if (!trace || (!h_diag && pg.n_s2)) why = "null pointer";
            else if (logn < 1 || logn > 32) why = "logn out of range";
            else if (trace_words != pg.W << logn) why = "trace_words must be W * 2^logn";
            else if (n_stage2 < 0 || (size_t)n_stage2 != pg.n_s2) why = "n_stage2 is not the program's";
            else why = nullptr;
        }
        if (why) {
            if (ctx) {
                try { ctx->err = std::string("bad argument: ") + why; } catch (...) {}
            }
            return ZP_ERR_ARG;
        }
        if (pg.n_s2 == 0) return ZP_OK;
        if (ctx) {
            if (!zpi_stage2_diag_device) { ctx->err = "this build has no device stage-2 diagnosis"; return ZP_ERR_UNSUPPORTED; }
            return zpi_stage2_diag_device(ctx, pg, (const u64 *)trace, logn, h_diag);
        }
        return diagnose_host(pg, (const u64 *)trace, logn, threads, h_diag);
    } catch (const std::bad_alloc &) {
        return ZP_ERR_NOMEM;
    } catch (...) {
        return ZP_ERR_INTERNAL;
    }
}
