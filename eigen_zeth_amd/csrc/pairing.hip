// The BN254 pairing behind the C ABI and the Groth16 verifier on top of it: zp_pairing_bn254, zp_pairing_check_bn254, zp_groth16_verify,
// zp_groth16_verify_batch (include/zeth_prover.h).  The arithmetic is csrc/pairing254.hpp; this file is the loops that run its two units of work
// on host threads, and the verifier's bookkeeping.
//   a job     one (G1, G2) pair as it crossed the ABI -> range, curve, twist and subgroup checks, the Miller value (108 Montgomery words) and a
//             status byte (p12_job).  A refused pair runs the same fixed loop on the generators.
//   a finish  one group of k consecutive Miller values: their product, times one more value (the key's e(-alpha, beta), made once per call), then
//             either the raw product (the reduction round of zp_pairing_check_bn254), or the final exponentiation and the GT words, or the byte
//             "is one" (p12_finish).
// EVERYTHING HERE RUNS ON THE HOST, with or without a ctx.  The two units are shaped as one-lane-per-job kernels (fixed trip counts, branches on
// constants only, no lane touching another's slots), but no kernel is launched: DESIGN.md section 3 says why.
// The checker's statement of the same mathematics: oracle/bn254_pairing.py, oracle/groth16_verify.py.
#include <cstring>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "pairing254.hpp"

namespace {

enum { FINISH_RAW = 0, FINISH_GT = 1, FINISH_IS_ONE = 2 };

// group g of `k` consecutive values out of n (the last group may be short); what is written depends on the mode
P12_FN void p12_finish(const u32 *vals, size_t n, size_t k, size_t g, const u32 *extra, int mode, u32 *out, unsigned char *is_one) {
    const size_t first = g * k, cnt = n - first < k ? n - first : k;
    fq12 acc, e;
    p12_group_product(acc, vals + 108 * first, cnt, extra);
    if (mode == FINISH_RAW) {
        fq12_store(acc, out + 108 * g);
        return;
    }
    fq12_final_exp(e, acc);
    if (mode == FINISH_GT) fq12_to_flat_words(e, out + 96 * g);
    else is_one[g] = fq12_is_one(e) ? 1 : 0;
}

int host_threads(int threads, size_t items) {
    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T = T < 1 ? 1 : T > 16 ? 16 : T;
    if ((size_t)T > items) T = (int)(items ? items : 1);
    return T;
}
// The work of every entry point: n jobs -> Miller values and status bytes; then the values in groups of k (k = 0: ONE group of all n, reduced in
// one round over the threads), each finished in `mode` with `extra`.  out: u32[groups][96] (FINISH_GT) or unused; is_one: u8[groups] (FINISH_IS_ONE).
int32_t pairing_run(const u32 *g1, const u32 *g2, const unsigned char *flags, size_t n, int threads, size_t k, const u32 *extra, int mode,
                    u32 *out, unsigned char *is_one, unsigned char *status) {
    if (n == 0) return ZP_OK;
    const bool one_group = k == 0;
    std::vector<u32> vals(n * 108), tmp;
    zpi_split_over_threads(n, host_threads(threads, n), [&](size_t a, size_t b) {
        for (size_t j = a; j < b; j++) {
            fq12 f;
            status[j] = (unsigned char)p12_job(g1 + 16 * j, g2 + 32 * j, flags ? flags[j] : 0u, f);
            fq12_store(f, vals.data() + 108 * j);
        }
    });
    size_t count = n;
    if (one_group) {
        const int T = host_threads(threads, n / 2);
        const size_t kr = (count + T - 1) / T;
        if (T > 1 && kr < count) {                         // one round: every thread multiplies its share
            const size_t groups = (count + kr - 1) / kr;
            tmp.resize(groups * 108);
            zpi_split_over_threads(groups, (int)groups, [&](size_t a, size_t b) {
                for (size_t g = a; g < b; g++) p12_finish(vals.data(), count, kr, g, nullptr, FINISH_RAW, tmp.data(), nullptr);
            });
            vals.swap(tmp);
            count = groups;
        }
    }
    const size_t kk = one_group ? count : k, groups = (count + kk - 1) / kk;
    zpi_split_over_threads(groups, host_threads(threads, groups), [&](size_t a, size_t b) {
        for (size_t g = a; g < b; g++) p12_finish(vals.data(), count, kk, g, extra, mode, out, is_one);
    });
    return ZP_OK;
}

// ---- the verifier's host side
void neg_words(const u32 *in, u32 *out) {   // -v mod q on eight standard-form words (v < q)
    fq_to_words(fq_neg(fq_from_words(in)), out);
}
// 0 valid (infinity included), else the status of p12_job, without a Miller loop: what a key's points are judged by, once per call
u32 g1_status(const u32 *w) {
    if (!p12_words_lt_q(w) || !p12_words_lt_q(w + 8)) return 1;
    if (p12_words_zero(w, 16)) return 0;
    return g1_on_curve(fq_to_mont(fq_from_words(w)), fq_to_mont(fq_from_words(w + 8))) ? 0 : 2;
}
u32 g2_status(const u32 *w) {
    for (int k = 0; k < 4; k++)
        if (!p12_words_lt_q(w + 8 * k)) return 1;
    if (p12_words_zero(w, 32)) return 0;
    const fq2 x = f_to_mont(FT<fq2>::from_words(w)), y = f_to_mont(FT<fq2>::from_words(w + 16));
    if (!g2_on_twist(x, y)) return 2;
    return g2_in_subgroup(x, y) ? 0 : 3;
}
const u32 FR_R_WORDS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
bool scalar_lt_r(const uint64_t *s) {
    for (int i = 3; i >= 0; i--) {
        const uint64_t r = (uint64_t)FR_R_WORDS[2 * i] | ((uint64_t)FR_R_WORDS[2 * i + 1] << 32);
        if (s[i] != r) return s[i] < r;
    }
    return false;
}
// out = IC_0 + sum_j pub_j IC_j as an affine point of the ABI (all-zero = infinity); the key's points are valid, the scalars < r
void ic_sum(const u32 *ic, int n_ic, const uint64_t *pub, u32 *out) {
    jacT<fq> acc = jac_inf<fq>();
    for (int j = 0; j < n_ic; j++) {
        const u32 *w = ic + 16 * (size_t)j;
        if (p12_words_zero(w, 16)) continue;
        const fq x = fq_to_mont(fq_from_words(w)), y = fq_to_mont(fq_from_words(w + 8));
        if (j == 0) {
            acc = jac_madd(acc, x, y);
            continue;
        }
        const uint64_t *s = pub + 4 * (size_t)(j - 1);
        jacT<fq> t = jac_inf<fq>();
        for (int i = 255; i >= 0; i--) {
            t = jac_dbl(t);
            if ((s[i >> 6] >> (i & 63)) & 1) t = jac_madd(t, x, y);
        }
        acc = jac_add(acc, t);
    }
    if (fq_is_zero(acc.Z)) memset(out, 0, 64);
    else jac_affine_words(acc, fq_inv_host(acc.Z), out);
}

constexpr int VK_HEAD = 16 + 3 * 32;   // alpha1 | beta2 | gamma2 | delta2, then ic[n_ic][16]

int32_t groth16_verify_all(zp_ctx *ctx, const u32 *vk, int32_t n_ic, const u32 *proofs, const uint64_t *publics, size_t n, int32_t threads,
                           int32_t *verdicts) {
    if (!vk || n_ic < 1 || (n && (!proofs || !verdicts)) || (n && n_ic > 1 && !publics)) {
        if (ctx) ctx->err = "bad argument: zp_groth16_verify: null pointer or n_ic < 1";
        return ZP_ERR_ARG;
    }
    // the key, once per call: every point valid, none of alpha, beta, gamma, delta at infinity (the equation would not bind the proof)
    bool key_ok = g1_status(vk) == 0 && !p12_words_zero(vk, 16);
    for (int k = 0; k < 3; k++) key_ok = key_ok && g2_status(vk + 16 + 32 * k) == 0 && !p12_words_zero(vk + 16 + 32 * k, 32);
    for (int j = 0; key_ok && j < n_ic; j++) key_ok = g1_status(vk + VK_HEAD + 16 * (size_t)j) == 0;
    if (!key_ok) {
        if (ctx) ctx->err = "bad argument: zp_groth16_verify: a point of the key is invalid, or alpha / beta / gamma / delta is at infinity";
        return ZP_ERR_ARG;
    }
    if (n == 0) return ZP_OK;
    // e(-alpha, beta) as a Miller value, and -gamma, -delta:  e(A, B) e(X, -gamma) e(C, -delta) e(-alpha, beta) = 1
    u32 nalpha[16], ngamma[32], ndelta[32], extra[108];
    memcpy(nalpha, vk, 64);
    neg_words(vk + 8, nalpha + 8);
    memcpy(ngamma, vk + 48, 128);
    neg_words(vk + 48 + 16, ngamma + 16);
    neg_words(vk + 48 + 24, ngamma + 24);
    memcpy(ndelta, vk + 80, 128);
    neg_words(vk + 80 + 16, ndelta + 16);
    neg_words(vk + 80 + 24, ndelta + 24);
    {
        fq12 f;
        (void)p12_job(nalpha, vk + 16, P12_SKIP_SUBGROUP, f);
        fq12_store(f, extra);
    }
    const size_t npub = (size_t)n_ic - 1;
    std::vector<u32> g1(n * 3 * 16, 0), g2(n * 3 * 32, 0);
    std::vector<unsigned char> flags(n * 3, P12_SKIP_SUBGROUP), status(n * 3, 0), is_one(n, 0), pub_bad(n, 0);
    zpi_split_over_threads(n, host_threads(threads, n), [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const uint64_t *pub = publics ? publics + 4 * npub * i : nullptr;
            for (size_t j = 0; j < npub; j++)
                if (!scalar_lt_r(pub + 4 * j)) pub_bad[i] = 1;
            if (pub_bad[i]) continue;        // its three jobs stay at infinity: computed like every other, and discarded
            const u32 *pr = proofs + 64 * i;
            memcpy(&g1[(3 * i) * 16], pr, 64);
            memcpy(&g2[(3 * i) * 32], pr + 16, 128);
            flags[3 * i] = 0;                // pi_b is the one G2 point nobody has checked
            ic_sum(vk + VK_HEAD, n_ic, pub, &g1[(3 * i + 1) * 16]);
            memcpy(&g2[(3 * i + 1) * 32], ngamma, 128);
            memcpy(&g1[(3 * i + 2) * 16], pr + 48, 64);
            memcpy(&g2[(3 * i + 2) * 32], ndelta, 128);
        }
    });
    ZP_TRY(pairing_run(g1.data(), g2.data(), flags.data(), 3 * n, threads, 3, extra, FINISH_IS_ONE, nullptr, is_one.data(), status.data()));
    for (size_t i = 0; i < n; i++) {
        if (pub_bad[i]) verdicts[i] = ZP_VERDICT_PUBLICS;
        else if (status[3 * i] || status[3 * i + 1] || status[3 * i + 2]) verdicts[i] = ZP_VERDICT_POINT;
        else verdicts[i] = is_one[i] ? ZP_VERDICT_ACCEPT : ZP_VERDICT_PAIRING;
    }
    return ZP_OK;
}

}  // namespace

extern "C" {

int32_t zp_pairing_bn254(zp_ctx *ctx, const uint32_t *h_g1, const uint32_t *h_g2, size_t n, int32_t threads, uint32_t *h_gt, uint8_t *h_status) {
    try {
        if (n == 0) return ZP_OK;
        if (!h_g1 || !h_g2 || !h_gt || !h_status) {
            if (ctx) ctx->err = "bad argument: zp_pairing_bn254: null pointer";
            return ZP_ERR_ARG;
        }
        ZP_TRY(pairing_run(h_g1, h_g2, nullptr, n, threads, 1, nullptr, FINISH_GT, h_gt, nullptr, h_status));
        for (size_t j = 0; j < n; j++)
            if (h_status[j]) memset(h_gt + 96 * j, 0, 384);
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

int32_t zp_pairing_check_bn254(zp_ctx *ctx, const uint32_t *h_g1, const uint32_t *h_g2, size_t n, int32_t threads, int32_t *ok) {
    try {
        if (!ok || (n && (!h_g1 || !h_g2))) {
            if (ctx) ctx->err = "bad argument: zp_pairing_check_bn254: null pointer";
            return ZP_ERR_ARG;
        }
        *ok = 1;
        if (n == 0) return ZP_OK;
        std::vector<unsigned char> status(n, 0);
        unsigned char is_one = 0;
        ZP_TRY(pairing_run(h_g1, h_g2, nullptr, n, threads, 0, nullptr, FINISH_IS_ONE, nullptr, &is_one, status.data()));
        for (size_t j = 0; j < n; j++)
            if (status[j]) is_one = 0;
        *ok = is_one;
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

int32_t zp_groth16_verify(zp_ctx *ctx, const uint32_t *h_vk, int32_t n_ic, const uint32_t *h_proof, const uint64_t *h_publics, int32_t *verdict) {
    try {
        return groth16_verify_all(ctx, h_vk, n_ic, h_proof, h_publics, 1, 0, verdict);
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

int32_t zp_groth16_verify_batch(zp_ctx *ctx, const uint32_t *h_vk, int32_t n_ic, const uint32_t *h_proofs, const uint64_t *h_publics, size_t n,
                                int32_t threads, int32_t *verdicts) {
    try {
        return groth16_verify_all(ctx, h_vk, n_ic, h_proofs, h_publics, n, threads, verdicts);
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

}  // extern "C"
