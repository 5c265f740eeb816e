// One Groth16 proof of the wrap circuit behind one call (GenFinalProof, proto/prover/v1/prover.proto:130-148; src/prover/provider.rs:472-503):
// witness completion + A w, B w, C w on the GPU (zp_r1cs_eval_device, csrc/r1cs.hip), the QAP quotient (csrc/ntt_bn254.hip), five MSMs over the
// key's points in HBM (csrc/msm.hip), the blinding terms -> the three proof elements.  The caller-set wires come from zp_wrap_assign
// (csrc/wrap_assign.hip).
#include <chrono>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "r1cs_circuit.hpp"

using namespace r1cs;

namespace {

// out[k] = w[wires[k]]: the scalars of an MSM over the key points of a SUBSET of the wires (those with a non-zero column in B)
__global__ void __launch_bounds__(256) r1cs_gather_kernel(const u64 *__restrict__ w, const u32 *__restrict__ wires, size_t n, u64 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 j = wires[i];
#pragma unroll
    for (int k = 0; k < 4; k++) out[i * 4 + k] = w[j * 4 + k];
}

// zp_groth16_prove, and with a communicator its sharded form (zp_groth16_prove_sharded): comm == nullptr is the one-ctx proof; otherwise every key
// array is this rank's slice (zpi_shard_range over the array the one-ctx proof reads), the five local partial sums are exchanged in one all-gather
// and added in rank order, and everything else runs replicated.
int32_t groth16_prove_impl(zp_ctx *ctx, zp_comm *comm, const uint64_t *circ, size_t words, const uint32_t *d_u1x, const uint32_t *d_v_wires, size_t n_v,
                           const uint32_t *d_v1x, const uint32_t *d_v2x, const uint32_t *d_l1, const uint32_t *d_h1, const uint32_t *h_delta1,
                           const uint64_t *set_idx, const uint64_t *set_val, size_t n_set, const uint64_t *h_r, const uint64_t *h_s, uint32_t *out_a,
                           uint32_t *out_b, uint32_t *out_c, uint64_t *out_pub, double *h_ms, int64_t *bad) {
    if (!ctx) return ZP_ERR_ARG;
    ZP_BIND(ctx);
    Circ c;
    ZP_ARG(ctx, parse(circ, words, &c), "malformed circuit blob");
    const size_t n = c.n_wires, m = (size_t)1 << c.logm;
    // the slices of this rank (first, count) over the five point arrays: A (n + 2), B in G1 and G2 (n_v + 2), l (n), h (m - 1); the whole arrays on one ctx
    const int world = comm ? zp_comm_world(comm) : 1, rank = comm ? zp_comm_rank(comm) : 0;
    size_t f0 = 0, k0 = n + 2, f1 = 0, k1 = n_v + 2, f3 = 0, k3 = n, f4 = 0, k4 = m - 1;
    if (comm) {
        zpi_shard_range(n + 2, world, rank, &f0, &k0);
        zpi_shard_range(n_v + 2, world, rank, &f1, &k1);
        zpi_shard_range(n, world, rank, &f3, &k3);
        zpi_shard_range(m - 1, world, rank, &f4, &k4);
    }
    const size_t kv = f1 < n_v ? (f1 + k1 < n_v ? k1 : n_v - f1) : 0;          // entries of d_v_wires in this slice (the rest are the tail's 1 and s)
    if (!comm)
        ZP_ARG(ctx, d_u1x && d_v_wires && n_v >= 1 && n_v <= c.n_wires && d_v1x && d_v2x && d_l1 && d_h1 && h_delta1 && set_idx && set_val && h_r && h_s && out_a && out_b && out_c && out_pub, "null argument");
    else
        ZP_ARG(ctx, (!k0 || d_u1x) && (!kv || d_v_wires) && n_v >= 1 && n_v <= c.n_wires && (!k1 || (d_v1x && d_v2x)) && (!k3 || d_l1) && (!k4 || d_h1) && h_delta1 && set_idx &&
                    set_val && h_r && h_s && out_a && out_b && out_c && out_pub, "null argument (a key slice this rank owns, or another pointer)");
    ZP_ARG(ctx, fr_is_canonical_u64(h_r) && fr_is_canonical_u64(h_s), "blinding scalars must be below the group order");
    if (bad) *bad = -1;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    void *d_abc = nullptr, *d_sc = nullptr, *d_tail = nullptr, *d_x = nullptr;
    const size_t abc_bytes = 3 * m * 32, sc_bytes = (n + 2 + n_v + 2) * 32, tail_bytes = 5 * (64 + 32), x_bytes = comm ? (size_t)(world + 1) * 96 * 4 : 0;
    int32_t rc = ZP_OK;
    try {
        ZP_TRY(zpi_pool_alloc(ctx, abc_bytes, &d_abc));
        rc = zpi_pool_alloc(ctx, sc_bytes, &d_sc);
        if (rc == ZP_OK) rc = zpi_pool_alloc(ctx, tail_bytes, &d_tail);
        if (rc == ZP_OK && comm) rc = zpi_pool_alloc(ctx, x_bytes, &d_x);
        auto done = [&](int32_t r) {
            if (d_abc) zpi_pool_release(ctx, d_abc, abc_bytes);
            if (d_sc) zpi_pool_release(ctx, d_sc, sc_bytes);
            if (d_tail) zpi_pool_release(ctx, d_tail, tail_bytes);
            if (d_x) zpi_pool_release(ctx, d_x, x_bytes);
            return r;
        };
        if (rc != ZP_OK) return done(rc);
        uint64_t *da = (uint64_t *)d_abc, *db = da + 4 * m, *dc = db + 4 * m;
        // the witness is completed where the MSMs read it: [w | 1 | r or s] (two extra scalars for the blinding terms that ride in the MSMs)
        if ((rc = zp_r1cs_eval_device(ctx, circ, words, set_idx, set_val, n_set, (uint64_t *)d_sc, da, db, dc, out_pub, bad)) != ZP_OK) return done(rc);
        uint64_t ext[8] = {1, 0, 0, 0, h_r[0], h_r[1], h_r[2], h_r[3]};
        if ((rc = zpi_h2d_small(ctx, (uint64_t *)d_sc + 4 * n, ext, 64)) != ZP_OK) return done(rc);
        uint64_t *d_scv = (uint64_t *)d_sc + 4 * (n + 2);                          // [w_j of the wires in B | 1 | s] -- of this rank's slice
        if (kv)
            hipLaunchKernelGGL(r1cs_gather_kernel, dim3((unsigned)((kv + 255) / 256)), dim3(256), 0, ctx->stream, (const u64 *)d_sc, d_v_wires, kv, (u64 *)d_scv);
        memcpy(ext + 4, h_s, 32);
        if (f1 + k1 > n_v) {                                                      // the slice reaches the tail: its 1 and / or s
            const size_t j0 = f1 > n_v ? f1 : n_v;
            if ((rc = zpi_h2d_small(ctx, d_scv + 4 * (j0 - f1), ext + 4 * (j0 - n_v), (f1 + k1 - j0) * 32)) != ZP_OK) return done(rc);
        }
        const auto t1 = now();
        // H = (A B - C) / Z: its coefficients replace A's evaluations and are the scalars of the h MSM
        const uint64_t coset[4] = {7, 0, 0, 0};
        if ((rc = zp_qap_quotient_bn254(ctx, da, db, dc, (int32_t)c.logm, coset)) != ZP_OK) return done(rc);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "QAP step failed"; return done(ZP_ERR_HIP); }
        const auto t2 = now();
        uint32_t A1[16], B1[16], Cl[16], Ch[16];
        const uint32_t *sc = (const uint32_t *)d_sc;
        // The five MSMs are independent and, at 1-2 M points, each is a chain of short launches with two host round trips: they run on five
        // streams at once -- A on this ctx, the others on helper ctxs of their own (stream + Pippenger arena, kept for the life of the ctx);
        // everything they read was finished by the synchronisation above.  Knob g16_parallel (0: one after the other).
        int32_t rcs[5] = {ZP_OK, ZP_OK, ZP_OK, ZP_OK, ZP_OK};
        double tms[5] = {0, 0, 0, 0, 0};
        zp_ctx *hc[5] = {ctx, ctx, ctx, ctx, ctx};
        bool par = ctx->tune_g16_parallel != 0;
        for (int i = 0; par && i < 4; i++) {
            if (!ctx->msm_helpers[i] && zp_create(&ctx->msm_helpers[i], ctx->device) != ZP_OK) par = false;
            if (par) {
                ctx->msm_helpers[i]->tune_msm_c = ctx->tune_msm_c;
                ctx->msm_helpers[i]->tune_msm_chunk_log = ctx->tune_msm_chunk_log;
                hc[i + 1] = ctx->msm_helpers[i];
            }
        }
        if (!par) for (int i = 1; i < 5; i++) hc[i] = ctx;
        auto job = [&](int k) noexcept {       // runs on helper threads: nothing may escape (an exception there would end the process)
          try {
            const auto ta = now();
            switch (k) {
                case 0: rcs[0] = zp_msm_bn254(hc[0], d_u1x, sc + 8 * f0, k0, A1); break;                               // alpha + sum_j w_j u_j + r delta
                case 1: rcs[1] = zp_msm_bn254(hc[1], d_v1x, (const uint32_t *)d_scv, k1, B1); break;                   // beta + sum_j w_j v_j + s delta
                case 2: rcs[2] = zp_msm_bn254_g2(hc[2], d_v2x, (const uint32_t *)d_scv, k1, out_b); break;
                case 3: rcs[3] = zp_msm_bn254(hc[3], d_l1, sc + 8 * f3, k3, Cl); break;
                default: rcs[4] = zp_msm_bn254(hc[4], d_h1, (const uint32_t *)da + 8 * f4, k4, Ch); break;            // sum_i H_i [tau^i Z(tau) / delta]
            }
            tms[k] = ms(ta, now());
          } catch (...) {
            rcs[k] = ZP_ERR_INTERNAL;
          }
        };
        if (par) {
            // a thread that cannot be started (EAGAIN) is not fatal: the ones already running are joined, the remaining MSMs run here
            std::thread th[4];
            int started = 0;
            try {
                for (int k = 1; k < 5; k++) { th[k - 1] = std::thread(job, k); started = k; }
            } catch (...) {
            }
            job(0);
            for (int k = started + 1; k < 5; k++) { hc[k] = ctx; job(k); }
            for (int k = 1; k <= started; k++) th[k - 1].join();
        } else {
            for (int k = 0; k < 5; k++) job(k);
        }
        for (int k = 0; k < 5; k++)
            if (rcs[k] != ZP_OK) {
                if (rcs[k] == ZP_ERR_INTERNAL && hc[k]->err.empty()) ctx->err = "exception in an MSM of zp_groth16_prove";
                else if (hc[k] != ctx) ctx->err = hc[k]->err;
                return done(rcs[k]);
            }
        if (comm) {
            // this rank's five partial sums [A | B1 | B (G2) | l | h] (96 words) to every rank in one all-gather; the sums in rank order on the host
            uint32_t *outs[5] = {A1, B1, out_b, Cl, Ch};
            const int pw[5] = {16, 16, 32, 16, 16}, at[5] = {0, 16, 32, 64, 80};
            std::vector<uint32_t> all((size_t)world * 96), one((size_t)world * 32);
            for (int k = 0; k < 5; k++) memcpy(all.data() + at[k], outs[k], pw[k] * 4);
            if ((rc = zpi_h2d_small(ctx, d_x, all.data(), 96 * 4)) != ZP_OK) return done(rc);
            if ((rc = zp_comm_all_gather(comm, (const uint64_t *)d_x, (uint64_t *)d_x + 48, 48)) != ZP_OK) return done(rc);
            if ((rc = zpi_d2h_small(ctx, all.data(), (const uint64_t *)d_x + 48, (size_t)world * 96 * 4)) != ZP_OK) return done(rc);
            for (int k = 0; k < 5; k++) {
                for (int h = 0; h < world; h++) memcpy(one.data() + (size_t)h * pw[k], all.data() + (size_t)h * 96 + at[k], pw[k] * 4);
                zpi_bn254_affine_sum(pw[k] == 32, one.data(), world, outs[k]);
            }
        }
        // pi_c = Cl + Ch + s A + r B1 - r s delta: one more (five-point) MSM
        const Fr fr_r = fr_from_std(h_r), fr_s = fr_from_std(h_s);
        const Fr zero = {{0, 0, 0, 0}};
        uint64_t tsc[5][4] = {{1, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        memcpy(tsc[2], h_s, 32);
        memcpy(tsc[3], h_r, 32);
        fr_to_std(fr_sub(zero, fr_mul(fr_r, fr_s)), tsc[4]);
        uint32_t tpt[5][16];
        memcpy(tpt[0], Cl, 64); memcpy(tpt[1], Ch, 64); memcpy(tpt[2], A1, 64); memcpy(tpt[3], B1, 64); memcpy(tpt[4], h_delta1, 64);
        if ((rc = zpi_h2d_small(ctx, d_tail, tpt, sizeof tpt)) != ZP_OK) return done(rc);
        if ((rc = zpi_h2d_small(ctx, (uint8_t *)d_tail + sizeof tpt, tsc, sizeof tsc)) != ZP_OK) return done(rc);
        if ((rc = zp_msm_bn254(ctx, (const uint32_t *)d_tail, (const uint32_t *)((uint8_t *)d_tail + sizeof tpt), 5, out_c)) != ZP_OK) return done(rc);
        memcpy(out_a, A1, 64);
        if (h_ms) {
            h_ms[0] = ms(t0, t1); h_ms[1] = ms(t1, t2); h_ms[2] = ms(t2, now());
            for (int k = 0; k < 5; k++) h_ms[3 + k] = tms[k];       // each MSM on its own clock (they overlap; h_ms[2] is their wall time + the tail)
        }
        return done(ZP_OK);
    } catch (...) {
        if (d_abc) zpi_pool_release(ctx, d_abc, abc_bytes);
        if (d_sc) zpi_pool_release(ctx, d_sc, sc_bytes);
        if (d_tail) zpi_pool_release(ctx, d_tail, tail_bytes);
        if (d_x) zpi_pool_release(ctx, d_x, x_bytes);
        ctx->err = "out of host memory in zp_groth16_prove";
        return ZP_ERR_NOMEM;
    }
}
}  // namespace

extern "C" {

// One Groth16 proof.  circ: the circuit blob; d_u1x (G1, u32[n_wires + 2][16]): [u_j]_1 | alpha_1 | delta_1; d_v_wires u32[n_v]: the wires with a
// non-zero column in B, ascending (a third of the gadget's wires never stand in B: their key points would be infinity); d_v1x (G1, u32[n_v + 2][16]):
// [v_j]_1 of those wires | beta_1 | delta_1; d_v2x (G2, u32[n_v + 2][32]): [v_j]_2 of those wires | beta_2 | delta_2; d_l1 (G1, u32[n_wires][16], infinity at wire 0 and the public inputs: those are
// the verifier's); d_h1 (G1, u32[2^logm - 1][16]) -- device-resident key points in the MSM layout; h_delta1 u32[16].
// set_idx / set_val: the n_set caller-set wires (zp_wrap_assign; wire 0 = 1 among them).  h_r, h_s: the blinding scalars (4 words each, standard
// form).  out_a u32[16], out_b u32[32], out_c u32[16]: pi_a, pi_b, pi_c (affine, standard form); out_pub u64[n_pub][4]: the public inputs the proof
// is for; h_ms (may be NULL) double[8]: milliseconds of witness completion, QAP step, all MSMs, then the MSMs one by one (A, B in G1, B in G2, l, h).  -20 / -21 as zp_r1cs_eval (*bad): no proof for a
// false statement.
int32_t zp_groth16_prove(zp_ctx *ctx, const uint64_t *circ, size_t words, const uint32_t *d_u1x, const uint32_t *d_v_wires, size_t n_v, const uint32_t *d_v1x,
                         const uint32_t *d_v2x, const uint32_t *d_l1, const uint32_t *d_h1, const uint32_t *h_delta1, const uint64_t *set_idx, const uint64_t *set_val, size_t n_set,
                         const uint64_t *h_r, const uint64_t *h_s, uint32_t *out_a, uint32_t *out_b, uint32_t *out_c, uint64_t *out_pub, double *h_ms,
                         int64_t *bad) {
    return groth16_prove_impl(ctx, nullptr, circ, words, d_u1x, d_v_wires, n_v, d_v1x, d_v2x, d_l1, d_h1, h_delta1, set_idx, set_val, n_set, h_r, h_s, out_a, out_b,
                              out_c, out_pub, h_ms, bad);
}

// The same proof over the ranks of a communicator (include/zeth_prover.h): every key array is this rank's slice, the result is the same on every
// rank.  A rank whose own step fails takes the communicator down before it returns (its peers return ZP_ERR_COMM from the all-gather); -20 / -21 come
// from the replicated witness on every rank alike and leave the communicator usable.
int32_t zp_groth16_prove_sharded(zp_comm *comm, const uint64_t *circ, size_t words, const uint32_t *d_u1x, const uint32_t *d_v_wires, size_t n_v,
                                 const uint32_t *d_v1x, const uint32_t *d_v2x, const uint32_t *d_l1, const uint32_t *d_h1, const uint32_t *h_delta1,
                                 const uint64_t *set_idx, const uint64_t *set_val, size_t n_set, const uint64_t *h_r, const uint64_t *h_s, uint32_t *out_a,
                                 uint32_t *out_b, uint32_t *out_c, uint64_t *out_pub, double *h_ms, int64_t *bad) {
    zp_ctx *ctx = zpi_comm_ctx(comm);
    if (!ctx) return ZP_ERR_ARG;
    const int32_t rc = groth16_prove_impl(ctx, comm, circ, words, d_u1x, d_v_wires, n_v, d_v1x, d_v2x, d_l1, d_h1, h_delta1, set_idx, set_val, n_set, h_r, h_s,
                                          out_a, out_b, out_c, out_pub, h_ms, bad);
    return (rc == ZP_OK || rc == -20 || rc == -21) ? rc : zpi_comm_fail(comm, rc);
}

}  // extern "C"
