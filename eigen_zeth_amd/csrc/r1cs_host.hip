// R1CS over the BN254 scalar field for the Groth16 wrap of GenFinalProof (proto/prover/v1/prover.proto:130-148; consumer
// src/settlement/ethereum/mod.rs:338-394, interfaces/zkvm.rs:82-130) on the HOST: the witness programs of the arithmetic templates, witness
// completion with the evaluation vectors A w, B w, C w of the QAP step (what zp_qap_quotient_bn254 takes), and the key generator's scalars
// u_j(tau), v_j(tau), w_j(tau).  Everything runs over the templates per instance (csrc/r1cs_circuit.hpp: the blob, the walks, the row rule) --
// 23 M multiply-adds for 1 900 gadget instances: a second on one core, instances in parallel on threads.  The group operations (fixed-base
// multiplications for the key, MSMs for a proof) are the GPU's (csrc/msm.hip).  No device code: builds as plain C++ under the host sanitizers.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "r1cs_circuit.hpp"

using namespace r1cs;

namespace {

// ---- the witness programs of the arithmetic templates.  W u64[n_wires][4]: wire values in standard form; set[n_wires].
// value of combination `id` of instance `in` over W; false: it reads a wire nobody has set.  cf: the template's coefficients in Montgomery form
// (fr_mul(coefficient, standard-form wire) = the standard-form product)
inline bool arith_lc(const ArithT &t, const std::vector<Fr> &cf, const uint64_t *in, uint64_t id, const uint64_t *W, const uint8_t *set, Fr *out) {
    Fr acc = {{0, 0, 0, 0}};
    const bool ok = arith_terms(t, in, id, cf, [&](uint64_t g, const auto &coef) {
        if (!set[g]) return false;
        Fr w;
        memcpy(w.l, W + 4 * g, 32);
        acc = fr_add(acc, fr_mul(coef, w));
        return true;
    });
    *out = acc;
    return ok;
}
// a standard-form value < r mod the Goldilocks prime; with q: its quotient too
inline uint64_t divmod_gl(const Fr &v, uint64_t *q) {
    uint64_t rem = 0;
    for (int k = 3; k >= 0; k--) {
        const u128 cur = ((u128)rem << 64) | v.l[k];
        if (q) q[k] = (uint64_t)(cur / GL_P);
        rem = (uint64_t)(cur % GL_P);
    }
    return rem;
}
// runs the witness program of instance i: 0 = done, -20 = an op cannot be carried out (no witness: the statement is false), -21 = unset input
int32_t arith_witness(const ArithT &t, const std::vector<Fr> &cf, uint64_t i, uint64_t *W, uint8_t *set) {
    const uint64_t *in = t.instance(i);
    auto put = [&](uint64_t local, const uint64_t *v4) {
        const uint64_t g = t.global(in, local);
        memcpy(W + 4 * g, v4, 32);
        set[g] = 1;
    };
    for (uint64_t o = 0; o < t.n_ops; o++) {
        const uint64_t *op = t.ops + 4 * o;
        const uint64_t code = ar_op_code(op[0]), nbits = ar_op_nbits(op[0]), flag = ar_op_flag(op[0]), dst = op[1];
        auto operand = [&](int k, Fr *v) { return arith_lc(t, cf, in, ar_lc_id(op + 2, k), W, set, v); };
        Fr a, b, c3;
        if (!operand(0, &a)) return -21;
        if (code == AR_OP_MUL) {
            if (!operand(1, &b)) return -21;
            const Fr pr = fr_mul(fr_mul(a, FR_R2), b);
            put(dst, pr.l);
        } else if (code == AR_OP_DIVMOD) {
            uint64_t q[4];
            const uint64_t r4[4] = {divmod_gl(a, q), 0, 0, 0};
            if (flag == 2) {
                if (r4[0]) return -20;
                put(dst, q);
            } else {
                put(dst, q);
                put(dst + 1, r4);
            }
        } else if (code == AR_OP_BITS) {
            for (uint64_t k = nbits; k < 256; k++)
                if ((a.l[k >> 6] >> (k & 63)) & 1) return -20;
            for (uint64_t k = 0; k < nbits; k++) {
                const uint64_t v4[4] = {(a.l[k >> 6] >> (k & 63)) & 1, 0, 0, 0};
                put(dst + k, v4);
            }
        } else {        // AR_OP_INV3: y with x y = 1 in F_p[t] / (t^3 - t - 1), x = the three operands mod p
            if (!operand(1, &b) || !operand(2, &c3)) return -21;
            u64 det;
            const e3 adj = e3_adj(e3_make(divmod_gl(a, nullptr), divmod_gl(b, nullptr), divmod_gl(c3, nullptr)), &det);
            if (det == 0) return -20;
            const e3 y = e3_scale(adj, gl_inv(det));
            for (int k = 0; k < 3; k++) {
                const uint64_t v4[4] = {y.c[k], 0, 0, 0};
                put(dst + k, v4);
            }
        }
    }
    return ZP_OK;
}

}  // namespace

// a template's instances on threads: they read caller-set wires and wires of EARLIER templates, and write their own
int32_t zpi_arith_witness_all(const Circ &c, uint64_t *W, uint8_t *set, int64_t *bad) {
    for (const ArithT &t : c.ar) {
        const std::vector<Fr> cf = mont_table(t.coef, t.n_coef);
        std::atomic<int64_t> fail{-1};
        std::atomic<int32_t> code{ZP_OK};
        parallel_for(t.n_inst, 16, 0, [&](uint64_t i) {
            if (set[t.base(i)]) return;           // the caller brought this instance's wires (a complete witness)
            const int32_t rc = arith_witness(t, cf, i, W, set);
            if (rc != ZP_OK) {
                note_min(fail, (int64_t)t.row(i, 0));
                code.store(rc);
            }
        });
        if (fail.load() >= 0) { if (bad) *bad = fail.load(); return code.load(); }
    }
    return ZP_OK;
}

extern "C" {

// Completes and checks a witness.  witness u64[n_wires][4] (standard form): wire 0 = 1, the public inputs and every wire that is not internal
// to a gadget or arithmetic instance are set by the caller; set[n_wires] (bytes) says which.  The witness programs run first; then the internal
// wires of every gadget instance are computed wave by wave (a template constraint defines one: csrc/r1cs_circuit.hpp eval_row); a wire that is
// defined twice must agree.  Then EVERY constraint is checked.  a_ev / b_ev / c_ev u64[2^logm][4] receive A w, B w, C w per constraint (zero
// padded): the input of the QAP step.  Returns ZP_OK; -20 = the assignment does not satisfy the circuit (*bad = first violated constraint) --
// there is no proof for a false statement; -21 = a row reads a wire nobody has set (*bad = the row; a gadget instance with an unset INPUT: its
// first row), or a wire is left unset (*bad = the wire); -21 before -20; ZP_ERR_ARG = malformed blob.
int32_t zp_r1cs_eval(const uint64_t *circ, size_t words, uint64_t *witness, uint8_t *set, uint64_t *a_ev, uint64_t *b_ev, uint64_t *c_ev, int64_t *bad) {
    Circ c;
    if (!parse(circ, words, &c) || !witness || !set || !a_ev || !b_ev || !c_ev) return ZP_ERR_ARG;
    if (bad) *bad = -1;
    try {
        if (!c.ar.empty()) {
            for (uint64_t j = 0; j < c.n_wires; j++) if (set[j] && !fr_is_canonical_u64(witness + 4 * j)) return ZP_ERR_ARG;
            const int32_t arc = zpi_arith_witness_all(c, witness, set, bad);
            if (arc != ZP_OK) return arc;
        }
        std::vector<Fr> w(c.n_wires);
        for (uint64_t j = 0; j < c.n_wires; j++)
            if (set[j]) {
                if (!fr_is_canonical_u64(witness + 4 * j)) return ZP_ERR_ARG;
                w[j] = fr_from_std(witness + 4 * j);
            }
        if (!set[0] || !fr_eq(w[0], FR_ONE)) return ZP_ERR_ARG;
        const uint64_t m = 1ull << c.logm;
        memset(a_ev, 0, m * 32); memset(b_ev, 0, m * 32); memset(c_ev, 0, m * 32);
        std::atomic<int64_t> first_bad{-1}, unset{-1};
        // one row; false = it reads an unset wire: the caller notes it (a gadget or arithmetic instance is abandoned there)
        auto row = [&](auto &&terms, uint64_t gdef, uint64_t r) {
            const RowResult res = eval_row(terms, gdef, w.data(), set, r, a_ev, b_ev, c_ev);
            if (res == ROW_BAD) note_min(first_bad, (int64_t)r);
            return res != ROW_UNSET;
        };
        // instances of one wave read only wires set before it and define disjoint (their own internal) wires: threads
        const std::vector<Fr> tv[3] = {mont_table(c.T[0].val, c.T[0].ptr[c.tc]), mont_table(c.T[1].val, c.T[1].ptr[c.tc]), mont_table(c.T[2].val, c.T[2].ptr[c.tc])};
        for (uint64_t wv = 0; wv < c.n_waves; wv++) {
            parallel_for(c.waves[wv + 1] - c.waves[wv], 32, 4, [&](uint64_t j) {
                const uint64_t i = c.waves[wv] + j, *in = c.instance(i);
                for (uint64_t k = 0; k < c.t; k++) if (!set[in[k]]) { note_min(unset, (int64_t)(i * c.tc)); return; }
                for (uint64_t q = 0; q < c.tc; q++) {
                    const uint64_t gdef = c.tdef[q] == ~0ull ? ~0ull : c.global(in, c.tdef[q]);
                    if (!row([&](int k, auto &&f) { return gadget_terms(c, in, q, k, tv[k], f); }, gdef, i * c.tc + q)) { note_min(unset, (int64_t)(i * c.tc + q)); return; }
                }
            });
            if (unset.load() >= 0) { if (bad) *bad = unset.load(); return -21; }
        }
        const MontAtUse ev[3] = {{c.E[0].val}, {c.E[1].val}, {c.E[2].val}};
        for (uint64_t q = 0; q < c.n_extra; q++)          // in order: an explicit row may define a wire
            if (!row([&](int k, auto &&f) { return explicit_terms(c, q, k, ev[k], f); }, c.edef[q], c.extra_base() + q)) {
                if (bad) *bad = (int64_t)(c.extra_base() + q);
                return -21;
            }
        for (const ArithT &t : c.ar) {          // (their wires are all set: the witness programs ran first)
            const std::vector<Fr> cm = mont_table(t.coef, t.n_coef);
            parallel_for(t.n_inst, 32, 0, [&](uint64_t i) {
                const uint64_t *in = t.instance(i);
                for (uint64_t q = 0; q < t.n_rows; q++)
                    if (!row([&](int k, auto &&f) { return arith_terms(t, in, ar_lc_id(ar_row(t.rows, q), k), cm, f); }, ~0ull, t.row(i, q))) { note_min(unset, (int64_t)t.row(i, q)); return; }
            });
            if (unset.load() >= 0) { if (bad) *bad = unset.load(); return -21; }
        }
        for (uint64_t j = 0; j < c.n_wires; j++) {
            if (!set[j]) { if (bad) *bad = (int64_t)j; return -21; }
            fr_to_std(w[j], witness + 4 * j);
        }
        if (first_bad.load() >= 0) { if (bad) *bad = first_bad.load(); return -20; }
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

// The scalars of a Groth16 key for this circuit at the point tau (a LOCAL, seeded setup: toxic waste known -- test keys, not a ceremony):
// with L_i the Lagrange basis of the 2^logm-th roots of unity (root 5^((r-1)/2^logm), the snarkjs / circom convention),
//   u_j = sum_i A[i][j] L_i(tau), v_j = sum_i B[i][j] L_i(tau), w_j = sum_i C[i][j] L_i(tau)            out_u, out_v u64[n_wires][4]
//   l_j = (beta u_j + alpha v_j + w_j) / delta for private wires, / gamma for wire 0 and the public inputs   out_l u64[n_wires][4]
//   h_i = tau^i (tau^m - 1) / delta, i < m - 1                                                              out_h u64[2^logm - 1][4]
// params u64[5][4]: tau, alpha, beta, gamma, delta (standard form).  The group elements are these scalars times the generators:
// zp_fixed_base_mul_bn254 / _g2.
int32_t zp_r1cs_key_scalars(const uint64_t *circ, size_t words, const uint64_t *params, uint64_t *out_u, uint64_t *out_v, uint64_t *out_l, uint64_t *out_h,
                            int32_t threads) {
    Circ c;
    if (!parse(circ, words, &c) || !params || !out_u || !out_v || !out_l || !out_h) return ZP_ERR_ARG;
    for (int k = 0; k < 5; k++) if (!fr_is_canonical_u64(params + 4 * k)) return ZP_ERR_ARG;
    try {
        const Fr tau = fr_from_std(params), alpha = fr_from_std(params + 4), beta = fr_from_std(params + 8), gamma = fr_from_std(params + 12),
                 delta = fr_from_std(params + 16);
        if (fr_is_zero(gamma) || fr_is_zero(delta)) return ZP_ERR_ARG;
        const uint64_t m = 1ull << c.logm;
        const Fr omega = fr_root_of_unity((unsigned)c.logm);
        // L_i(tau) = (tau^m - 1) w^i / (m (tau - w^i)): batch inversion of (tau - w^i)
        std::vector<Fr> L(m), pre(m);
        Fr wi = FR_ONE, run = FR_ONE;
        for (uint64_t i = 0; i < m; i++) {
            L[i] = fr_sub(tau, wi);
            if (fr_is_zero(L[i])) return ZP_ERR_ARG;               // tau on the domain: not a usable point
            pre[i] = run;
            run = fr_mul(run, L[i]);
            wi = fr_mul(wi, omega);
        }
        Fr tm = tau;
        for (uint64_t s = 0; s < c.logm; s++) tm = fr_mul(tm, tm);
        const Fr zt = fr_sub(tm, FR_ONE);
        const uint64_t mm[4] = {m, 0, 0, 0};
        const Fr scale = fr_mul(zt, fr_inv(fr_from_std(mm)));
        Fr inv = fr_inv(run);
        {
            std::vector<Fr> wpow(m);
            Fr x = FR_ONE;
            for (uint64_t i = 0; i < m; i++) { wpow[i] = x; x = fr_mul(x, omega); }
            for (uint64_t i = m; i-- > 0;) {
                const Fr d = fr_mul(inv, pre[i]);                   // 1 / (tau - w^i)
                inv = fr_mul(inv, L[i]);
                L[i] = fr_mul(fr_mul(scale, wpow[i]), d);
            }
        }
        const Fr zero = {{0, 0, 0, 0}};
        std::vector<Fr> acc[3];
        for (int k = 0; k < 3; k++) acc[k].assign(c.n_wires, zero);
        // every term (wire g, coefficient) of combination k of row i adds coefficient L_i to acc[k][g]
        auto scatter = [&](int k, const Fr &Li) { return [&acc, &Li, k](uint64_t g, const auto &coef) { acc[k][g] = fr_add(acc[k][g], fr_mul(coef, Li)); return true; }; };
        // gadget instances own their internal wires (no two write the same accumulator) but share input wires and the constant: a thread adds the
        // internal ones in place and keeps what it has for every other wire in a list of its chunk's, merged afterwards
        int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
        if (T < 1) T = 1;
        if (T > 32) T = 32;
        if ((uint64_t)T > c.n_inst) T = (int)(c.n_inst ? c.n_inst : 1);
        struct Shared { uint64_t g; int k; Fr v; };
        std::vector<std::vector<Shared>> side(T);
        const std::vector<Fr> tv[3] = {mont_table(c.T[0].val, c.T[0].ptr[c.tc]), mont_table(c.T[1].val, c.T[1].ptr[c.tc]), mont_table(c.T[2].val, c.T[2].ptr[c.tc])};
        parallel_for((uint64_t)T, T, 0, [&](uint64_t chunk) {
            for (uint64_t i = c.n_inst * chunk / T; i < c.n_inst * (chunk + 1) / T; i++) {
                const uint64_t *in = c.instance(i), base = c.base(i), n_int = c.n_int();
                for (int k = 0; k < 3; k++)
                    for (uint64_t q = 0; q < c.tc; q++) {
                        const Fr &Li = L[i * c.tc + q];
                        gadget_terms(c, in, q, k, tv[k], [&](uint64_t g, const Fr &coef) {
                            const Fr v = fr_mul(coef, Li);
                            if (g - base < n_int) acc[k][g] = fr_add(acc[k][g], v);
                            else side[chunk].push_back(Shared{g, k, v});
                            return true;
                        });
                    }
            }
        });
        for (const auto &lst : side)
            for (const Shared &e : lst) acc[e.k][e.g] = fr_add(acc[e.k][e.g], e.v);
        const MontAtUse ev[3] = {{c.E[0].val}, {c.E[1].val}, {c.E[2].val}};
        for (int k = 0; k < 3; k++)
            for (uint64_t q = 0; q < c.n_extra; q++) explicit_terms(c, q, k, ev[k], scatter(k, L[c.extra_base() + q]));
        for (const ArithT &t : c.ar) {          // instance by instance over the template's combinations
            const std::vector<Fr> cm = mont_table(t.coef, t.n_coef);
            for (uint64_t i = 0; i < t.n_inst; i++)
                for (uint64_t q = 0; q < t.n_rows; q++)
                    for (int k = 0; k < 3; k++) arith_terms(t, t.instance(i), ar_lc_id(ar_row(t.rows, q), k), cm, scatter(k, L[t.row(i, q)]));
        }
        const Fr dinv = fr_inv(delta), ginv = fr_inv(gamma);
        for (uint64_t j = 0; j < c.n_wires; j++) {
            fr_to_std(acc[0][j], out_u + 4 * j);
            fr_to_std(acc[1][j], out_v + 4 * j);
            const Fr l = fr_add(fr_add(fr_mul(beta, acc[0][j]), fr_mul(alpha, acc[1][j])), acc[2][j]);
            fr_to_std(fr_mul(l, j <= c.n_pub ? ginv : dinv), out_l + 4 * j);
        }
        Fr tp = fr_mul(zt, dinv);
        for (uint64_t i = 0; i + 1 < m; i++) { fr_to_std(tp, out_h + 4 * i); tp = fr_mul(tp, tau); }
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

}  // extern "C"
