// The caller-set wires of the Groth16 wrap circuit of GenFinalProof (proto/prover/v1/prover.proto:130-148; src/prover/provider.rs:472-503), on the
// HOST, from untrusted records:
//   zp_wrap_assign : the wires and their values from the binary openings of the final STARK (zp_stark_openings), driven by the assignment script
//                    the circuit builder writes beside the circuit blob (service/wrap_circuit.py: WrapCircuit.script)
//   zp_wrap_aux    : the aux list of a stage B-2 wrap (the statement's sparse fixed columns at zeta)
// zp_groth16_prove (csrc/groth16.hip) takes what zp_wrap_assign writes.  No device code: builds as plain C++ under the host sanitizers.
#include <cstdint>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "fr254_host.hpp"

namespace {

constexpr uint64_t SCRIPT_MAGIC = 0x3353504152575a50ULL;   // "PZWRAPS3" (round 6: challenge elements, a list of aux elements)
constexpr uint64_t OPEN_MAGIC = 0x33304e45504f5a50ULL;     // "PZOPEN03" (round 6: + the rate element behind every challenge)

struct OpenTree { uint64_t width, leaves, levels; const uint64_t *root; size_t off; };   // off: word offset of this tree's part inside a query record
struct Openings {
    uint64_t nq, ntr, logm;
    std::vector<OpenTree> tr;
    const uint64_t *q0;
    size_t qwords;
    // the transcript of the proof (round 5): every block of 16 field elements its sponge absorbed, in order, then the 16 rate elements of the
    // last absorbing permutation and of the squeeze-only permutations behind it (csrc/prove.hip writes them, service/wrap_circuit.py
    // TranscriptLog states them); 4 words per element
    uint64_t n_blocks, n_rates, n_chal;
    const uint64_t *blocks, *rates, *caps;      // caps: the capacity after every permutation (n_blocks + n_rates - 1 of them)
    const uint64_t *chal;                        // rate element 1 after every absorbed segment: what the challenge squeezed there is read from
    const uint64_t *query(uint64_t q) const { return q0 + q * qwords; }
};
bool parse_openings(const uint64_t *d, size_t words, Openings *o) {
    if (!d || words < 4 || d[0] != OPEN_MAGIC) return false;
    o->nq = d[1]; o->ntr = d[2]; o->logm = d[3];
    if (o->nq < 1 || o->nq > 4096 || o->ntr < 2 || o->ntr > 64 || o->logm > 40 || words < 4 + 7 * o->ntr) return false;
    size_t off = 1;
    o->tr.resize(o->ntr);
    for (uint64_t t = 0; t < o->ntr; t++) {
        OpenTree &T = o->tr[t];
        T.width = d[4 + 3 * t]; T.leaves = d[5 + 3 * t]; T.levels = d[6 + 3 * t];
        if (T.width < 1 || T.width > (1u << 16) || T.leaves < 1 || T.leaves > (1ull << 40) || (T.leaves & (T.leaves - 1)) || T.levels > 12) return false;
        T.root = d + 4 + 3 * o->ntr + 4 * t;
        T.off = off;
        off += T.width + T.levels * 64;
    }
    o->qwords = off;
    o->q0 = d + 4 + 7 * o->ntr;
    const size_t at = 4 + 7 * o->ntr + o->nq * off;
    if (words < at + 2) return false;
    o->n_blocks = d[at]; o->n_rates = d[at + 1];
    if (o->n_blocks < 1 || o->n_blocks > 4096 || o->n_rates < 1 || o->n_rates > 256) return false;
    o->blocks = d + at + 2;
    o->rates = o->blocks + o->n_blocks * 64;
    o->caps = o->rates + o->n_rates * 64;
    const size_t at2 = at + 2 + (o->n_blocks + o->n_rates) * 64 + (o->n_blocks + o->n_rates - 1) * 4;
    if (words < at2 + 1) return false;
    o->n_chal = d[at2];
    if (o->n_chal > 256) return false;
    o->chal = d + at2 + 1;
    return words == at2 + 1 + o->n_chal * 4;
}
inline uint64_t bit_of(const uint64_t *w4, unsigned i) { return (w4[i >> 6] >> (i & 63)) & 1; }      // bit i of a 4-word value

}  // namespace

extern "C" {

// script: [0] "PZWRAPS1" [1] entries [2] wires set in all [3] n_queries [4] n_trees [5] index bits, per tree (width, leaves, levels), then per entry six
// words: op, first wire, count, a, b, c --
//   0 constant a                      1 aux                                  2 root of tree b               3 index of query a
//   4 bits 0..count-1 of that index   5 elements of block c of the leaf (query a, tree b)                    6 the 16 digests of level c on the path
//   7 one-hot of the position at level c (16)       8 / 9 one-hot of its low / high two bits (4)
//   10 elements b .. b + count - 1 of absorbed block a of the transcript            11 the 16 rate elements of squeeze permutation a
//   12 bits c .. c + count - 1 of rate element b of squeeze permutation a           13 entries c .. of that element's "equal to r so far" chain
//      (walking down from bit 253 over the positions where r has a 1: the AND of the element's bits there, first position excluded)
//   14 the 30 partial products of the top 32 bits of 64-bit word c of that element (bits 32..33, 32..34, ... 32..62 of the word)
//   15 the capacity element after permutation a of the transcript (absorbing permutations in order, then the squeeze-only ones)
//   16 challenge element a (rate element 1 after absorbed segment a)               17 its low 192 bits (zeta as the circuit commits to it)
// aux u64[n_aux][4]: element 0 the value the proof is bound to (the aggregator address), elements 1.. whatever else the circuit takes from its
// caller (stage B-2: the statement's sparse fixed columns at zeta, one packed element each) -- op 1 reads element a.
// out_idx u64[cap], out_val u64[cap][4] (standard form) receive the wires and their values; *n_set their number ([2] of the script).
int32_t zp_wrap_assign(const uint64_t *script, size_t script_words, const uint64_t *openings, size_t open_words, const uint64_t *aux, size_t n_aux, uint64_t *out_idx,
                       uint64_t *out_val, size_t cap, size_t *n_set) {
    Openings o;
    if (!script || script_words < 6 || script[0] != SCRIPT_MAGIC || !aux || n_aux < 1 || !out_idx || !out_val || !n_set || !parse_openings(openings, open_words, &o))
        return ZP_ERR_ARG;
    const uint64_t ne = script[1], total = script[2];
    if (script[3] != o.nq || script[4] != o.ntr || script[5] != o.logm || ne > (1ull << 28) || script_words != 8 + 3 * o.ntr + 6 * ne || total > cap)
        return ZP_ERR_ARG;
    for (size_t i = 0; i < n_aux; i++) if (!fr_is_canonical_u64(aux + 4 * i)) return ZP_ERR_ARG;
    for (uint64_t i = 0; i < o.n_chal; i++) if (!fr_is_canonical_u64(o.chal + 4 * i)) return ZP_ERR_ARG;
    for (uint64_t t = 0; t < o.ntr; t++)
        if (script[6 + 3 * t] != o.tr[t].width || script[7 + 3 * t] != o.tr[t].leaves || script[8 + 3 * t] != o.tr[t].levels) return ZP_ERR_ARG;   // another layout
    if (script[6 + 3 * o.ntr] != o.n_blocks || script[7 + 3 * o.ntr] != o.n_rates) return ZP_ERR_ARG;                                              // another transcript
    for (uint64_t i = 0; i < (o.n_blocks + o.n_rates) * 16 + (o.n_blocks + o.n_rates - 1); i++)
        if (!fr_is_canonical_u64(o.blocks + 4 * i)) return ZP_ERR_ARG;
    // positions of r's one-bits below the top one, walking down: the chain of op 13
    unsigned ones[254], n_ones = 0;
    for (int i = 252; i >= 0; i--)
        if (bit_of(FR_MOD, (unsigned)i)) ones[n_ones++] = (unsigned)i;
    const uint64_t *e = script + 8 + 3 * o.ntr;
    size_t n = 0;
    for (uint64_t k = 0; k < ne; k++, e += 6) {
        const uint64_t op = e[0], wire = e[1], cnt = e[2], a = e[3], b = e[4], c = e[5];
        if (cnt < 1 || cnt > 64 || n + cnt > total || op > 17) return ZP_ERR_ARG;
        if (op >= 16) {                      // a challenge element, whole (16) or its low 192 bits (17)
            if (cnt != 1 || a >= o.n_chal) return ZP_ERR_ARG;
            out_idx[n] = wire;
            memcpy(out_val + 4 * n, o.chal + 4 * a, 32);
            if (op == 17) out_val[4 * n + 3] = 0;
            n++;
            continue;
        }
        if (op == 15) {                      // the capacity after permutation a of the transcript
            if (cnt != 1 || a >= o.n_blocks + o.n_rates - 1) return ZP_ERR_ARG;
            out_idx[n] = wire;
            memcpy(out_val + 4 * n, o.caps + 4 * a, 32);
            n++;
            continue;
        }
        if (op >= 10) {
            // (sums of script words are compared WITHOUT forming them: b + cnt wraps for a b near 2^64 -- found by tests/test_r1cs_fuzz.py, round 6)
            if (op == 10 ? (a >= o.n_blocks || b >= 16 || cnt > 16 - b) : a >= o.n_rates) return ZP_ERR_ARG;
            if ((op == 11 && cnt != 16) || (op >= 12 && b >= 16) || (op == 12 && (c >= 254 || cnt > 254 - c)) || (op == 13 && (c >= n_ones || cnt > n_ones - c)) ||
                (op == 14 && (cnt != 30 || c >= 3)))
                return ZP_ERR_ARG;
            const uint64_t *el = op == 10 ? o.blocks + (a * 16 + b) * 4 : o.rates + (a * 16 + (op == 11 ? 0 : b)) * 4;
            for (uint64_t i = 0; i < cnt; i++, n++) {
                uint64_t *v = out_val + 4 * n;
                out_idx[n] = wire + i;
                v[0] = v[1] = v[2] = v[3] = 0;
                if (op <= 11) memcpy(v, el + 4 * i, 32);
                else if (op == 12) v[0] = bit_of(el, (unsigned)(c + i));
                else if (op == 13) {
                    uint64_t p = bit_of(el, 253);
                    for (uint64_t t = 0; t <= c + i; t++) p &= bit_of(el, ones[t]);
                    v[0] = p;
                } else {
                    uint64_t p = 1;
                    for (uint64_t t = 0; t <= i + 1; t++) p &= bit_of(el, (unsigned)(64 * c + 32 + t));
                    v[0] = p;
                }
            }
            continue;
        }
        if (op >= 3 && a >= o.nq) return ZP_ERR_ARG;
        if (op == 1 && a >= n_aux) return ZP_ERR_ARG;
        if ((op == 2 || op >= 5) && b >= o.ntr) return ZP_ERR_ARG;
        const uint64_t *q = op >= 3 ? o.query(a) : nullptr;
        const OpenTree *T = (op == 2 || op >= 5) ? &o.tr[b] : nullptr;
        uint64_t pos = 0;
        if (op >= 6) {
            if (c >= T->levels) return ZP_ERR_ARG;
            pos = ((q[0] & (T->leaves - 1)) >> (4 * c)) & 15;
        }
        if ((op == 5 && (cnt != 16 || c >= (T->width + 55) / 56)) || ((op == 6 || op == 7) && cnt != 16) || (op >= 8 && cnt != 4) || (op == 4 && cnt > 64) ||
            ((op == 1 || op == 2 || op == 3) && cnt != 1))
            return ZP_ERR_ARG;
        for (uint64_t i = 0; i < cnt; i++, n++) {
            uint64_t *v = out_val + 4 * n;
            out_idx[n] = wire + i;
            v[0] = v[1] = v[2] = v[3] = 0;
            switch (op) {
                case 0: v[0] = a; break;
                case 1: memcpy(v, aux + 4 * a, 32); break;
                case 2: memcpy(v, T->root, 32); break;
                case 3: v[0] = q[0]; break;
                case 4: v[0] = (q[0] >> i) & 1; break;
                case 5: leaf_block_element((const u64 *)(q + T->off), 1, 0, (int)T->width, (int)(56 * c), (int)i, (u64 *)v); break;
                case 6: memcpy(v, q + T->off + T->width + (c * 16 + i) * 4, 32); break;
                case 7: v[0] = pos == i; break;
                case 8: v[0] = (pos & 3) == i; break;
                default: v[0] = (pos >> 2) == i; break;
            }
        }
    }
    if (n != total) return ZP_ERR_ARG;
    *n_set = n;
    return ZP_OK;
}

// The aux list of a stage B-2 wrap (zp_wrap_assign's `aux`) from what the host of GenFinalProof holds: the final STARK's openings record (its
// challenge element 1 IS zeta: three low 64-bit words, each mod p), the final STARK's statement (constraint program, public inputs, trace length,
// root of unity) and the element the proof is bound to.  out_aux u64[cap][4]: element 0 = addr4, element 1 + k = sparse fixed column k of the
// program at zeta, components packed c0 + c1 2^64 + c2 2^128; *n_aux = n_fixed - 1.  zeta3_out (may be NULL) u64[3]: the three WORDS zeta is read from.
int32_t zp_wrap_aux(const uint64_t *openings, size_t open_words, const uint64_t *h_program, size_t program_words, const uint64_t *h_pub, int32_t n_pub, int32_t logn,
                    uint64_t root32, const uint64_t *addr4, uint64_t *out_aux, size_t cap, size_t *n_aux, uint64_t *zeta3_out) {
    Openings o;
    if (!addr4 || !out_aux || !n_aux || !parse_openings(openings, open_words, &o) || o.n_chal < 2 || !fr_is_canonical_u64(addr4)) return ZP_ERR_ARG;
    uint64_t zeta[3];
    for (int k = 0; k < 3; k++) zeta[k] = o.chal[4 + k] % GL_P;
    try {
        // the one header word that sizes this call's arrays, by name; zp_program_fixed_eval_ext parses the blob (once) and refuses what it refuses
        if (!h_program || program_words < ZPH_WORDS) return ZP_ERR_ARG;
        const uint64_t n_fixed = h_program[ZPH_N_FIXED];
        if (n_fixed < 2 || n_fixed > 4096 || cap < n_fixed - 1) return ZP_ERR_ARG;
        std::vector<uint64_t> fixed(3 * n_fixed);
        const int32_t rc = zp_program_fixed_eval_ext(h_program, program_words, h_pub, n_pub, logn, root32, zeta, fixed.data(), (int32_t)n_fixed, 0);
        if (rc != ZP_OK) return rc;
        memcpy(out_aux, addr4, 32);
        for (uint64_t k = 2; k < n_fixed; k++) {
            uint64_t *e = out_aux + 4 * (k - 1);
            e[0] = fixed[3 * k]; e[1] = fixed[3 * k + 1]; e[2] = fixed[3 * k + 2]; e[3] = 0;
        }
        *n_aux = n_fixed - 1;
        if (zeta3_out) memcpy(zeta3_out, o.chal + 4, 24);       // the words as the circuit commits to them (a word >= p names its residue a second time)
        return ZP_OK;
    } catch (...) {
        return ZP_ERR_NOMEM;
    }
}

}  // extern "C"
