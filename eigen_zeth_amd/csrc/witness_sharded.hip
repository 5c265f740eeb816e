// The witness check over the ranks of a communicator: what the sharded provers run under "prove_check" (csrc/prove.hip) and what
// zp_stark_check_witness_sharded runs before a proof.  A rank holds COLUMNS of the trace (zpi_shard_range), a constraint reads ROWS, so:
//   canonical pass   every rank streams ITS words against p (zpi_witness_canonical); the (count, first word) pairs are all-gathered and every rank
//                    derives the same (sum, smallest GLOBAL word index c N + r) -- ranks own ascending column ranges, so that is the first word of
//                    the lowest rank that has any
//   exchange         the raw columns [wl][N] -> rows [G wl][N / G] (zp_exchange_columns_to_rows, the extension's exchange), one all-gather of every
//                    rank's first row (G x W words) for the halo: the window buffer is [W][N / G + 1].  Stage "witness_exchange".  G = 1: neither
//   constraints      the row-window kernel of the program or the interpreter (zpi_witness_launch with a window) on rows [rank N / G, (rank + 1) N / G)
//   merge            every rank's result [first key][first_row: K][counts: K] is all-gathered; zpi_witness_merge, then the report by the code that
//                    makes it for one GPU (csrc/witness_merge.hpp)
// Every decision to stop is taken from gathered data: all ranks stop at the same point.  A rank-local failure returns its error code; the entry
// points hand it to zpi_comm_fail, so no peer waits.
#include <hip/hip_runtime.h>

#include <vector>

#include "ctx.hpp"
#include "witness_merge.hpp"

namespace {

struct Pooled {          // a device buffer from the ctx pool, given back when the scope ends
    zp_ctx *ctx;
    void *p = nullptr;
    size_t bytes = 0;
    explicit Pooled(zp_ctx *c) : ctx(c) {}
    ~Pooled() { if (p) zpi_pool_release(ctx, p, bytes); }
    int32_t get(size_t words) {
        bytes = (words ? words : 1) * 8;
        return zpi_pool_alloc(ctx, bytes, &p);
    }
    u64 *w() const { return (u64 *)p; }
};

}  // namespace

// *bad_n = trace words >= p over all ranks, *bad_at = the GLOBAL index c N + r of the first in memory order (~0: none): the same on every rank
int32_t zpi_witness_sharded_canonical(zp_comm *comm, size_t W, int logn, const u64 *d_trace_local, u64 *bad_n, u64 *bad_at) {
    zp_ctx *ctx = zpi_comm_ctx(comm);
    const int G = zp_comm_world(comm), rank = zp_comm_rank(comm);
    const size_t N = (size_t)1 << logn, wl = (W + (size_t)G - 1) / (size_t)G;
    size_t first, wr;
    zpi_shard_range(W, G, rank, &first, &wr);
    u64 mine[2] = {0, ~0ULL};
    if (wr) ZP_TRY(zpi_witness_canonical(ctx, d_trace_local, wr * N, &mine[0], &mine[1]));
    Pooled d(ctx);
    ZP_TRY(d.get(2 + 2 * (size_t)G));
    ZP_TRY(zpi_h2d_small(ctx, d.w(), mine, 16));
    ZP_TRY(zp_comm_all_gather(comm, (const uint64_t *)d.w(), (uint64_t *)(d.w() + 2), 2));
    std::vector<u64> all(2 * (size_t)G);
    ZP_TRY(zpi_d2h_small(ctx, all.data(), d.w() + 2, all.size() * 8));
    *bad_n = 0; *bad_at = ~0ULL;
    for (int g = 0; g < G; g++) {
        if (all[2 * g] && *bad_at == ~0ULL) *bad_at = (u64)g * wl * N + all[2 * g + 1];
        *bad_n += all[2 * g];
    }
    return ZP_OK;
}

// the constraints over the ranks: d_s2 = the stage-2 columns on the trace domain, whole on every rank (NULL: the program has none); pubchal as
// zpi_witness_constraints takes it.  The same report, counts and first rows on every rank.  Requires 2^logn / world >= 2 (the callers check
// before their first collective) and canonical words (the field code takes nothing else).
int32_t zpi_witness_sharded_constraints(zp_comm *comm, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace_local,
                                        const u64 *d_s2, int logn, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row) {
    zp_ctx *ctx = zpi_comm_ctx(comm);
    const int G = zp_comm_world(comm), rank = zp_comm_rank(comm);
    const size_t N = (size_t)1 << logn, W = pg.W, K = pg.K, wl = (W + (size_t)G - 1) / (size_t)G, nl = N / (size_t)G;
    size_t first, wr;
    zpi_shard_range(W, G, rank, &first, &wr);
    ZP_ARG(ctx, nl >= 2, "the witness check over the ranks needs at least two trace rows per rank");
    Pooled cols(ctx), pack(ctx), rows(ctx), heads(ctx), allh(ctx), buf(ctx);
    ZpWitnessWindow win{N, 0, N};
    const u64 *window = d_trace_local;
    if (G > 1) {
        ZpStage stage_(ctx, "witness_exchange");
        const u64 *src = d_trace_local;
        if (wr < wl) {           // the exchange moves wl columns per rank: the missing ones as zeros (they land behind column W)
            ZP_TRY(cols.get(wl * N));
            ZP_TRY(zp_dev_zero(ctx, cols.w() + wr * N, (wl - wr) * N * 8));
            if (wr) ZP_TRY(zp_d2d(ctx, cols.w(), d_trace_local, wr * N * 8));
            src = cols.w();
        }
        ZP_TRY(pack.get(wl * N));
        ZP_TRY(rows.get((size_t)G * wl * nl));
        ZP_TRY(heads.get(W));
        ZP_TRY(allh.get((size_t)G * W));
        ZP_TRY(buf.get(W * (nl + 1)));
        ZP_TRY(zp_exchange_columns_to_rows(comm, (const uint64_t *)src, wl, N, (uint64_t *)pack.w(), (uint64_t *)rows.w()));      // [G wl][nl]: all columns, my rows
        ZP_HIP(ctx, hipMemcpy2DAsync(heads.w(), 8, rows.w(), nl * 8, 8, W, hipMemcpyDeviceToDevice, ctx->stream));                // my first row
        ZP_TRY(zp_comm_all_gather(comm, (const uint64_t *)heads.w(), (uint64_t *)allh.w(), W));
        ZP_HIP(ctx, hipMemcpy2DAsync(buf.w(), (nl + 1) * 8, rows.w(), nl * 8, nl * 8, W, hipMemcpyDeviceToDevice, ctx->stream));
        ZP_HIP(ctx, hipMemcpy2DAsync(buf.w() + nl, (nl + 1) * 8, allh.w() + (size_t)((rank + 1) % G) * W, 8, 8, W, hipMemcpyDeviceToDevice,
                                     ctx->stream));                                                                                // ... of the next rank
        win = ZpWitnessWindow{nl + 1, (size_t)rank * nl, nl};
        window = buf.w();
    }
    const size_t res_words = zpi_witness_result_words(K);
    Pooled res(ctx);
    ZP_TRY(res.get(res_words * (1 + (size_t)G)));
    ZP_TRY(zpi_witness_launch(ctx, pg, dg32, pubchal, window, d_s2, logn, &win, res.w()));
    ZP_TRY(zp_comm_all_gather(comm, (const uint64_t *)res.w(), (uint64_t *)(res.w() + res_words), res_words));
    std::vector<u64> parts(res_words * (size_t)G), merged(res_words);
    ZP_TRY(zpi_d2h(ctx, parts.data(), res.w() + res_words, parts.size() * 8));
    zpi_witness_merge((const uint64_t *)parts.data(), (size_t)G, K, (uint64_t *)merged.data());
    zpi_witness_report((const uint64_t *)merged.data(), K, h_report, h_counts, h_first_row);
    return ZP_OK;
}

// The stage-2 columns of a column-sharded trace, whole on every rank: a broadcast of the (at most three) witness columns an argument reads from the
// rank that owns them, then the prover's primitives at the challenge g.  d_s2 u64[W2][N]; d_colb: scratch of 3 N words.  The sharded prover and
// zp_stark_check_witness_sharded both make them here.
int32_t zpi_stage2_columns_sharded(zp_comm *comm, const ZpProgram &pg, const u64 *d_trace_local, int logn, const u64 g[3], u64 *d_colb, u64 *d_s2) {
    zp_ctx *ctx = zpi_comm_ctx(comm);
    const int G = zp_comm_world(comm), rank = zp_comm_rank(comm);
    const size_t N = (size_t)1 << logn, wl = (pg.W + (size_t)G - 1) / (size_t)G;
    auto column = [&](u64 idx, u64 *dst) -> int32_t {       // broadcast from the rank that owns it
        const int owner = (int)(idx / wl);
        if (owner == rank) ZP_TRY(zp_d2d(ctx, dst, d_trace_local + (idx % wl) * N, N * 8));
        return zp_comm_broadcast(comm, (uint64_t *)dst, N, owner);
    };
    size_t at = 0;
    for (size_t k = 0; k < pg.n_s2; k++) {
        const u64 *st = pg.stage2 + 4 * k;
        for (size_t j = 0; j < zpi_stage2_inputs(st[0]); j++) ZP_TRY(column(st[1 + j], d_colb + j * N));
        ZP_TRY(zpi_stage2_argument(ctx, st, d_colb, d_colb + N, d_colb + 2 * N, N, g, d_s2, &at));
    }
    return ZP_OK;
}

namespace {

int32_t check_sharded(zp_comm *comm, zp_ctx *ctx, const ZpProgram &pg, const uint64_t *h_program, size_t program_words, const std::vector<u64> &pubchal,
                      const u64 *d_trace_local, int logn, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row) {
    const size_t N = (size_t)1 << logn;
    u64 bad_n, bad_at;
    ZP_TRY(zpi_witness_sharded_canonical(comm, pg.W, logn, d_trace_local, &bad_n, &bad_at));
    if (bad_n != 0) {        // the same on every rank: nobody goes on to the exchange
        zpi_witness_noncanonical_report(pg.K, N, bad_n, bad_at, h_report, h_counts, h_first_row);
        return ZP_OK;
    }
    Pooled s2(ctx), colb(ctx);
    if (pg.n_s2) {
        ZP_TRY(s2.get(pg.W2 * N));
        ZP_TRY(colb.get(3 * N));
        ZpStage stage_(ctx, "witness_stage2");
        ZP_TRY(zpi_stage2_columns_sharded(comm, pg, d_trace_local, logn, pubchal.data() + pg.n_pub, colb.w(), s2.w()));
    }
    uint8_t dg[32];
    const bool lookup = ctx->tune_witness_kernel && !ctx->air_kernels.empty();
    if (lookup) zpi_program_digest_cached(ctx, h_program, program_words, dg);
    return zpi_witness_sharded_constraints(comm, pg, lookup ? dg : nullptr, pubchal, d_trace_local, pg.n_s2 ? s2.w() : nullptr, logn, h_report, h_counts,
                                           h_first_row);
}

}  // namespace

extern "C" int32_t zp_stark_check_witness_sharded(zp_comm *comm, const uint64_t *h_program, size_t program_words, const uint64_t *d_trace_local, size_t trace_words,
                                                  const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, const uint64_t *h_chal3, uint64_t *h_report,
                                                  uint64_t *h_counts, uint64_t *h_first_row, int32_t n_constraints) {
    if (!comm) return ZP_ERR_ARG;
    zp_ctx *ctx = zpi_comm_ctx(comm);
    int32_t rc;
    try {
        ZP_BIND(ctx);
        ZpProgram pg;
        std::vector<u64> pubchal;
        const int G = zp_comm_world(comm);
        const char *why = zpi_witness_args(h_program, program_words, d_trace_local, trace_words, G, zp_comm_rank(comm), h_pubs, n_pubs, logn, h_chal3,
                                           h_report, h_counts, h_first_row, n_constraints, &pg, &pubchal);
        if (!why && logn > 30) why = "logn out of range";
        if (!why && ((size_t)1 << logn) / (size_t)G < 2) why = "the witness check over the ranks needs at least two trace rows per rank";
        if (why) {
            ctx->err = std::string("bad argument: ") + why;
            rc = ZP_ERR_ARG;
        } else {
            rc = check_sharded(comm, ctx, pg, h_program, program_words, pubchal, (const u64 *)d_trace_local, logn, h_report, h_counts, h_first_row);
        }
    } catch (const std::bad_alloc &) {
        rc = ZP_ERR_NOMEM;
    } catch (...) {
        rc = ZP_ERR_INTERNAL;
    }
    return zpi_comm_fail(comm, rc);      // a rank that stops alone (its arguments, an allocation, a launch) frees its peers
}
