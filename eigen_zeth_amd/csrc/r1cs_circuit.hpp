// The R1CS circuit blob (layout: eigen_zeth_amd/service/r1cs.py pack_circuit, service/arith.py) as the library holds it, read ONCE: the parsed
// form and its validator, the accessors of every packed field (GL_HD: the kernels of csrc/r1cs.hip decode the blob in HBM through the same ones),
// one walk over the terms of a row per row kind, and THE rule of a row (eval_row).  csrc/r1cs_host.hip evaluates, generates key scalars and runs
// the witness programs over these; csrc/r1cs.hip is the device evaluator; csrc/groth16.hip the prover.  Builds as plain C++ for the host sanitizers.
//
// A circuit that verifies the hashing of a STARK is thousands of copies of ONE gadget (a width-17 Poseidon-BN254 permutation: 613 constraints over
// 631 local wires, about 12 000 matrix entries) plus a few ten thousand glue constraints, so the matrices are never materialised: the gadget is a
// TEMPLATE (three sparse matrices over local wires), an instance is a map of its inputs + the base of its internal wires, the glue comes as
// explicit sparse rows, and the Goldilocks arithmetic of the verifier as arithmetic templates.  Rows: gadget instances first (instance i owns
// [i tc, (i + 1) tc)), then the explicit rows, then the arithmetic templates' (instance i of a template owns first_row + [i n_rows, (i + 1) n_rows)).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <thread>
#include <vector>

#include "fr254_host.hpp"

// ---- the packed fields
// a combination id: bit 31 set = the unit combination of one local wire, else an index into the template's pool of combinations
constexpr uint32_t AR_UNIT = 1u << 31;
GL_HD bool lc_is_unit(u64 id) { return (id & AR_UNIT) != 0; }
GL_HD u64 lc_unit_wire(u64 id) { return id & (AR_UNIT - 1); }
// an arithmetic row is two words, A | B << 32 and C (words 2 and 3 of a witness op hold its operands the same way): combination k = 0, 1, 2
template <class W> GL_HD const W *ar_row(const W *rows, u64 q) { return rows + 2 * q; }
template <class W> GL_HD u64 ar_lc_id(const W *row, int k) { return k == 0 ? row[0] & 0xFFFFFFFFull : k == 1 ? row[0] >> 32 : row[1]; }
// a pool entry: local wire | coefficient index << 32
GL_HD u64 ar_ent_wire(u64 ent) { return ent & 0xFFFFFFFFull; }
GL_HD u64 ar_ent_coef(u64 ent) { return ent >> 32; }
// a witness op is four words: code | nbits << 8 | flag << 24, first wire it defines, operands (above)
enum { AR_OP_MUL = 1, AR_OP_DIVMOD = 3, AR_OP_BITS = 4, AR_OP_INV3 = 5 };
GL_HD u64 ar_op_code(u64 w) { return w & 0xFF; }
GL_HD u64 ar_op_nbits(u64 w) { return (w >> 8) & 0xFFFF; }
GL_HD u64 ar_op_flag(u64 w) { return (w >> 24) & 0xFF; }
// an instance record, of the gadget (n_in = t; one more word behind: its first row) and of an arithmetic template alike: the wires of its n_in
// inputs, then the base of its internal wires.  Local wire 0 is the constant, 1..n_in the inputs, the internal ones follow.
template <class W> GL_HD const W *ar_instance(const W *inst, u64 n_in, u64 i) { return inst + i * (n_in + 1); }     // (an arithmetic template's)
template <class W> GL_HD u64 local_to_global(const W *in, u64 n_in, u64 local) {
    return local == 0 ? 0 : local <= n_in ? in[local - 1] : in[n_in] + (local - 1 - n_in);
}

namespace r1cs {

constexpr uint64_t MAGIC = 0x3130534331525a50ULL;   // "PZR1CS01"
constexpr uint64_t MAGIC2 = 0x3230534331525a50ULL;  // "PZR1CS02": + the arithmetic templates (service/arith.py) behind the explicit constraints
struct Mat { const uint64_t *ptr, *idx, *val; };      // CSR over constraints: ptr[n + 1], idx[nnz] (wire), val[nnz][4] (standard form)
// An arithmetic template (service/arith.py: Goldilocks arithmetic of the final STARK's verifier inside F_r, wrap stage B-2): rows over LOCAL wires
// as triples of combination ids into one pool, a witness program that DEFINES every internal wire, and n_inst instances.
struct ArithT {
    uint64_t n_in, n_int, n_coef, n_lc, nnz, n_rows, n_ops, n_inst, first_row;
    const uint64_t *coef, *lc_ptr, *lc_ent, *rows, *ops, *inst;
    uint64_t n_local() const { return 1 + n_in + n_int; }
    const uint64_t *instance(uint64_t i) const { return ar_instance(inst, n_in, i); }
    uint64_t base(uint64_t i) const { return instance(i)[n_in]; }          // first internal wire of instance i
    uint64_t row(uint64_t i, uint64_t q) const { return first_row + i * n_rows + q; }
    uint64_t global(const uint64_t *in, uint64_t local) const { return local_to_global(in, n_in, local); }
};
struct Circ {
    std::vector<ArithT> ar;
    uint64_t n_arith_rows = 0;
    uint64_t n_wires, n_cons, logm, t, n_local, tc, n_inst, n_extra, n_pub, n_waves;
    // tdef[tc]: the local wire a template constraint defines (~0: none); inst: (t + 2) words each; edef[n_extra]: the wire an explicit row defines;
    // waves[n_waves + 1]: instances [waves[k], waves[k + 1]) read only wires set before wave k
    const uint64_t *tdef, *inst, *edef, *waves;
    Mat T[3], E[3];
    uint64_t n_int() const { return n_local - 1 - t; }
    const uint64_t *instance(uint64_t i) const { return inst + i * (t + 2); }
    uint64_t base(uint64_t i) const { return instance(i)[t]; }
    uint64_t global(const uint64_t *in, uint64_t local) const { return local_to_global(in, t, local); }
    uint64_t extra_base() const { return n_inst * tc; }
};

namespace {      // (the rest is per translation unit: the walks and the row rule inline into their callers' loops)

inline bool parse_mat(const uint64_t *d, size_t words, size_t &at, uint64_t rows, uint64_t max_idx, Mat *m) {
    if (at + rows + 1 > words) return false;
    m->ptr = d + at;
    at += rows + 1;
    const uint64_t nnz = m->ptr[rows];
    if (m->ptr[0] != 0 || nnz > (1ull << 32) || at + nnz + 4 * nnz > words) return false;
    for (uint64_t i = 0; i < rows; i++) if (m->ptr[i] > m->ptr[i + 1]) return false;
    m->idx = d + at; at += nnz;
    m->val = d + at; at += 4 * nnz;
    for (uint64_t k = 0; k < nnz; k++) if (m->idx[k] >= max_idx || !fr_is_canonical_u64(m->val + 4 * k)) return false;
    return true;
}

inline bool parse_arith(const uint64_t *d, size_t words, size_t &at, uint64_t n_tpl, Circ *c) {
    uint64_t next_row = c->n_inst * c->tc + c->n_extra;
    for (uint64_t k = 0; k < n_tpl; k++) {
        if (at + 12 > words) return false;
        ArithT t;
        t.n_in = d[at]; t.n_int = d[at + 1]; t.n_coef = d[at + 2]; t.n_lc = d[at + 3]; t.nnz = d[at + 4]; t.n_rows = d[at + 5]; t.n_ops = d[at + 6]; t.n_inst = d[at + 7];
        t.first_row = d[at + 8];
        at += 12;
        if (t.n_in > (1u << 20) || t.n_int < 1 || t.n_int > (1u << 26) || t.n_coef > (1u << 24) || t.n_lc < 1 || t.n_lc > (1u << 28) || t.nnz > (1ull << 30) || t.n_rows < 1 ||
            t.n_rows > (1u << 26) || t.n_ops > (1u << 26) || t.n_inst < 1 || t.n_inst > (1u << 16) || t.first_row != next_row)
            return false;
        const uint64_t nl = t.n_local();
        if (nl >= AR_UNIT) return false;
        const uint64_t need = 4 * t.n_coef + (t.n_lc + 1) + t.nnz + 2 * t.n_rows + 4 * t.n_ops + t.n_inst * (t.n_in + 1);
        if (at + need > words) return false;
        t.coef = d + at; at += 4 * t.n_coef;
        t.lc_ptr = d + at; at += t.n_lc + 1;
        t.lc_ent = d + at; at += t.nnz;
        t.rows = d + at; at += 2 * t.n_rows;
        t.ops = d + at; at += 4 * t.n_ops;
        t.inst = d + at; at += t.n_inst * (t.n_in + 1);
        for (uint64_t i = 0; i < t.n_coef; i++) if (!fr_is_canonical_u64(t.coef + 4 * i)) return false;
        if (t.lc_ptr[0] != 0 || t.lc_ptr[t.n_lc] != t.nnz || t.lc_ptr[1] != 0) return false;           // LC 0 is the empty combination
        for (uint64_t i = 0; i < t.n_lc; i++) if (t.lc_ptr[i] > t.lc_ptr[i + 1]) return false;
        for (uint64_t e = 0; e < t.nnz; e++) if (ar_ent_wire(t.lc_ent[e]) >= nl || ar_ent_coef(t.lc_ent[e]) >= t.n_coef) return false;
        auto lc_ok = [&](uint64_t id) { return lc_is_unit(id) ? lc_unit_wire(id) < nl && id < (1ull << 32) : id < t.n_lc; };
        auto lcs_ok = [&](const uint64_t *row) { return lc_ok(ar_lc_id(row, 0)) && lc_ok(ar_lc_id(row, 1)) && lc_ok(ar_lc_id(row, 2)); };
        for (uint64_t q = 0; q < t.n_rows; q++) if (!lcs_ok(ar_row(t.rows, q))) return false;
        for (uint64_t o = 0; o < t.n_ops; o++) {
            const uint64_t *op = t.ops + 4 * o;
            const uint64_t code = ar_op_code(op[0]), nbits = ar_op_nbits(op[0]), flag = ar_op_flag(op[0]), dst = op[1];
            uint64_t cnt = 1;
            if (code == AR_OP_MUL) cnt = 1;
            else if (code == AR_OP_DIVMOD) { if (flag != 0 && flag != 2) return false; cnt = flag == 2 ? 1 : 2; }
            else if (code == AR_OP_BITS) { if (nbits < 1 || nbits > 254) return false; cnt = nbits; }
            else if (code == AR_OP_INV3) cnt = 3;
            else return false;
            if (dst < 1 + t.n_in || dst + cnt > nl) return false;                                        // an op defines INTERNAL wires
            if (!lcs_ok(op + 2)) return false;
        }
        for (uint64_t i = 0; i < t.n_inst; i++) {
            const uint64_t *in = t.instance(i);
            for (uint64_t j = 0; j < t.n_in; j++) if (in[j] >= c->n_wires) return false;
            if (t.base(i) + t.n_int > c->n_wires || t.base(i) < 1 + c->n_pub) return false;
        }
        next_row += t.n_inst * t.n_rows;
        c->n_arith_rows += t.n_inst * t.n_rows;
        c->ar.push_back(t);
    }
    return true;
}

inline bool parse(const uint64_t *d, size_t words, Circ *c) {
    if (!d || words < 16 || (d[0] != MAGIC && d[0] != MAGIC2)) return false;
    const uint64_t n_tpl = d[0] == MAGIC2 ? d[11] : 0;
    if (n_tpl > 16) return false;
    c->ar.clear();
    c->n_arith_rows = 0;
    c->n_wires = d[1]; c->n_cons = d[2]; c->logm = d[3]; c->t = d[4]; c->n_local = d[5]; c->tc = d[6]; c->n_inst = d[7]; c->n_extra = d[8]; c->n_pub = d[9];
    c->n_waves = d[10];
    if (c->n_wires < 2 || c->n_wires > (1ull << 28) || c->logm > 28 || c->t < 2 || c->t > 64 || c->n_local < 1 + c->t || c->n_local > (1u << 20) || c->tc < 1 ||
        c->tc > (1u << 20) || c->n_inst > (1u << 24) || c->n_extra > (1ull << 28) || c->n_pub < 1 || 1 + c->n_pub > c->n_wires)
        return false;
    if (c->n_cons < c->n_inst * c->tc + c->n_extra || c->n_cons > (1ull << c->logm)) return false;
    size_t at = 16;
    if (at + c->tc > words) return false;
    c->tdef = d + at; at += c->tc;
    for (uint64_t i = 0; i < c->tc; i++) if (c->tdef[i] != ~0ull && (c->tdef[i] < 1 + c->t || c->tdef[i] >= c->n_local)) return false;
    for (int k = 0; k < 3; k++) if (!parse_mat(d, words, at, c->tc, c->n_local, &c->T[k])) return false;
    if (at + c->n_inst * (c->t + 2) > words) return false;
    c->inst = d + at; at += c->n_inst * (c->t + 2);
    for (uint64_t i = 0; i < c->n_inst; i++) {
        const uint64_t *in = c->instance(i);
        for (uint64_t k = 0; k < c->t; k++) if (in[k] >= c->n_wires) return false;
        if (c->base(i) + c->n_int() > c->n_wires || in[c->t + 1] != i * c->tc) return false;
    }
    if (c->n_waves < 1 || c->n_waves > c->n_inst + 1 || at + c->n_waves + 1 > words) return false;
    c->waves = d + at; at += c->n_waves + 1;
    if (c->waves[0] != 0 || c->waves[c->n_waves] != c->n_inst) return false;
    for (uint64_t k = 0; k < c->n_waves; k++) if (c->waves[k] > c->waves[k + 1]) return false;
    if (at + c->n_extra > words) return false;
    c->edef = d + at; at += c->n_extra;
    for (uint64_t q = 0; q < c->n_extra; q++) if (c->edef[q] != ~0ull && c->edef[q] >= c->n_wires) return false;
    for (int k = 0; k < 3; k++) if (!parse_mat(d, words, at, c->n_extra, c->n_wires, &c->E[k])) return false;
    if (!parse_arith(d, words, at, n_tpl, c)) return false;
    return at == words && c->n_cons == c->n_inst * c->tc + c->n_extra + c->n_arith_rows;
}

// ---- the terms of combination k (0 A, 1 B, 2 C) of a row, one walk per row kind: f(global wire, coefficient) for every term, until f says
// false (the walk's result then).  The coefficient is what the CALLER's table `coef` holds at the term's index (every user converts the blob's
// coefficients to Montgomery form once per call), FrUnit for the unit combinations of an arithmetic row.
template <class Tab, class F> inline bool gadget_terms(const Circ &c, const uint64_t *in, uint64_t q, int k, const Tab &coef, F &&f) {
    for (uint64_t e = c.T[k].ptr[q]; e < c.T[k].ptr[q + 1]; e++) if (!f(c.global(in, c.T[k].idx[e]), coef[e])) return false;
    return true;
}
template <class Tab, class F> inline bool explicit_terms(const Circ &c, uint64_t q, int k, const Tab &coef, F &&f) {
    for (uint64_t e = c.E[k].ptr[q]; e < c.E[k].ptr[q + 1]; e++) if (!f(c.E[k].idx[e], coef[e])) return false;
    return true;
}
template <class Tab, class F> inline bool arith_terms(const ArithT &t, const uint64_t *in, uint64_t id, const Tab &coef, F &&f) {
    if (lc_is_unit(id)) return f(t.global(in, lc_unit_wire(id)), FrUnit{});
    for (uint64_t e = t.lc_ptr[id]; e < t.lc_ptr[id + 1]; e++) if (!f(t.global(in, ar_ent_wire(t.lc_ent[e])), coef[ar_ent_coef(t.lc_ent[e])])) return false;
    return true;
}
// coefficient tables: n values of the blob (standard form) in Montgomery form, made once per call; or converted at each use (the explicit rows:
// every entry is used once)
inline std::vector<Fr> mont_table(const uint64_t *val, uint64_t n) {
    std::vector<Fr> m(n);
    for (uint64_t i = 0; i < n; i++) m[i] = fr_from_std(val + 4 * i);
    return m;
}
struct MontAtUse { const uint64_t *val; Fr operator[](uint64_t e) const { return fr_from_std(val + 4 * e); } };

// THE rule of a row, whatever its kind (terms(k, f): one of the walks above).  Over w (Montgomery form) and set: the three combinations are
// summed; a term over an unset wire ends the row as ROW_UNSET with nothing stored -- except that a row which DEFINES wire gdef (~0: none) skips
// gdef in C while it is unset (its coefficient there is 1), sets w[gdef] = A B - (rest of C) and stores A B as C.  Every other row is checked,
// A B = C, and stored (standard form) whether it holds or not: ROW_BAD.
enum RowResult { ROW_OK, ROW_UNSET, ROW_BAD };
template <class Terms> inline RowResult eval_row(Terms &&terms, uint64_t gdef, Fr *w, uint8_t *set, uint64_t row, uint64_t *a_ev, uint64_t *b_ev, uint64_t *c_ev) {
    Fr s[3];
    for (int k = 0; k < 3; k++) {
        Fr acc = {{0, 0, 0, 0}};
        if (!terms(k, [&](uint64_t g, const auto &coef) {
                if (!set[g]) return k == 2 && g == gdef;
                acc = fr_add(acc, fr_mul(coef, w[g]));
                return true;
            }))
            return ROW_UNSET;
        s[k] = acc;
    }
    const Fr ab = fr_mul(s[0], s[1]);
    bool holds = true;
    if (gdef != ~0ull && !set[gdef]) {
        w[gdef] = fr_sub(ab, s[2]);
        set[gdef] = 1;
        s[2] = ab;
    } else {
        holds = fr_eq(ab, s[2]);
    }
    fr_to_std(s[0], a_ev + 4 * row); fr_to_std(s[1], b_ev + 4 * row); fr_to_std(s[2], c_ev + 4 * row);
    return holds ? ROW_OK : ROW_BAD;
}

// ---- threads: body(i) for every i < count on at most max_threads threads (and no more than the machine has) that take the next index from a
// counter; in order on the calling thread when there is one thread, or fewer than serial_below items
template <class Body> inline void parallel_for(uint64_t count, int max_threads, uint64_t serial_below, Body &&body) {
    uint64_t T = std::thread::hardware_concurrency();
    if (T > (uint64_t)max_threads) T = (uint64_t)max_threads;
    if (T > count) T = count;
    if (T <= 1 || count < serial_below) {
        for (uint64_t i = 0; i < count; i++) body(i);
        return;
    }
    std::atomic<uint64_t> next{0};
    auto loop = [&]() { for (;;) { const uint64_t i = next.fetch_add(1); if (i >= count) return; body(i); } };
    std::vector<std::thread> pool;
    for (uint64_t k = 0; k < T; k++) pool.emplace_back(loop);
    for (auto &th : pool) th.join();
}
// slot = the smallest index noted so far (-1: none)
inline void note_min(std::atomic<int64_t> &slot, int64_t v) {
    int64_t cur = slot.load();
    while ((cur < 0 || v < cur) && !slot.compare_exchange_weak(cur, v)) {}
}

}  // namespace
}  // namespace r1cs

// The witness programs of the arithmetic templates (csrc/r1cs_host.hip), for the device evaluator too: every instance of every template whose
// internal wires the caller did not set, in blob order.  W u64[n_wires][4]: wire values in standard form; set[n_wires].  ZP_OK; -20 = an op cannot
// be carried out (no witness: the statement is false), -21 = an op reads an unset wire; *bad: the first row of the first such instance.
int32_t zpi_arith_witness_all(const r1cs::Circ &c, uint64_t *W, uint8_t *set, int64_t *bad);
