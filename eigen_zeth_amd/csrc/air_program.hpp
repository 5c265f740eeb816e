// The ZPAIR1 constraint program (include/zeth_prover.h "constraint program"; layout: stark/air.py compile_program), read ONCE: the blob's field
// offsets and magic, the parsed form, the one validator, the decoder of an instruction word and of a sparse-column entry, and the one walk over
// the instruction stream (device: csrc/stark.hip on the LDE domain; host: csrc/witness_host.hip over the base field, csrc/verify.hip over
// F_{p^3}; csrc/witness_check.hip keeps its own loop over the field accessors below: its header says why).
// Usable from device translation units and from the host-only ones that build as plain C++ under the host sanitizers (gl.hpp's GL_HD convention);
// everything here is inline or a template.
//
//   word 0 magic | 1 W | 2 W2 | 3 n_fixed | 4 n_pub | 5 n_chal | 6 n_const | 7 n_instr | 8 K | 9 n_slots | 10 n_s2 | 11 Q
//   constants[n_const] | instructions[n_instr] | stage-2 table[n_s2][4] | per sparse fixed column: lp | n_entries << 8, then n_entries x (entry, value)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "gl.hpp"

enum : size_t { ZPH_MAGIC = 0, ZPH_W, ZPH_W2, ZPH_N_FIXED, ZPH_N_PUB, ZPH_N_CHAL, ZPH_N_CONST, ZPH_N_INSTR, ZPH_K, ZPH_N_SLOTS, ZPH_N_S2, ZPH_Q, ZPH_WORDS };
inline bool zpi_program_magic_ok(const uint64_t *blob) {
    static const unsigned char magic[8] = {'Z', 'P', 'A', 'I', 'R', '1', 0, 0};
    return memcmp(blob, magic, 8) == 0;
}

// ---- instruction word: op | dst << 8 | kind a << 24 | index a << 28 | kind b << 44 | index b << 48
enum : int { ZPI_ADD = 1, ZPI_SUB = 2, ZPI_MUL = 3, ZPI_OUT = 4 };     // slot[dst] = a op b;  OUT: constraint k = a (dst and b ignored)
// operand kinds: a slot, a committed column at this row / the next row, a fixed column, a public input or challenge word, a constant, x - w^(N-1)
enum : int { ZPK_SLOT = 0, ZPK_COL = 1, ZPK_NEXT = 2, ZPK_FIXED = 3, ZPK_PUB = 4, ZPK_CONST = 5, ZPK_XML = 6, ZPK_KINDS = 7 };
struct ZpInstr { int op, dst, kind[2], idx[2]; };
GL_HD int zpi_op(u64 w) { return (int)(w & 0xFF); }
GL_HD int zpi_dst(u64 w) { return (int)((w >> 8) & 0xFFFF); }
GL_HD int zpi_kind(u64 w, int o) { return (int)((w >> (24 + 20 * o)) & 0xF); }       // operand o = 0 (a), 1 (b)
GL_HD int zpi_idx(u64 w, int o) { return (int)((w >> (28 + 20 * o)) & 0xFFFF); }
GL_HD ZpInstr zpi_decode(u64 w) { return ZpInstr{zpi_op(w), zpi_dst(w), {zpi_kind(w, 0), zpi_kind(w, 1)}, {zpi_idx(w, 0), zpi_idx(w, 1)}}; }

// ---- stage-2 table: (kind, three trace columns) per argument.  A grand product reads two of them (a, b) and makes 3 planes (Z in F_{p^3}); LogUp
// reads three (a, t, m) and makes 9 (h1, h2, S).  The kind test of every reader (W2 below, the columns themselves in csrc/stage2.hip)
enum : u64 { ZPS2_PRODUCT = 1, ZPS2_LOGUP = 2 };
GL_HD size_t zpi_stage2_inputs(u64 kind) { return kind == ZPS2_PRODUCT ? 2 : 3; }
GL_HD size_t zpi_stage2_planes(u64 kind) { return kind == ZPS2_PRODUCT ? 3 : 9; }

// ---- the sparse periodic fixed columns (2 .. n_fixed - 1): the table behind the stage-2 table
struct ZpFixedCol { int lp; size_t first_entry_word, n_entries; bool has_pub; };
struct ZpFixedEntry { u64 pos; bool is_pub; u64 value; };       // value: the constant, or (is_pub) the index of the public input that stands there
inline ZpFixedEntry zpi_fixed_entry(const uint64_t *blob, const ZpFixedCol &fc, size_t e) {
    const u64 a = blob[fc.first_entry_word + 2 * e];
    return ZpFixedEntry{a & ~(1ULL << 63), (a >> 63) != 0, blob[fc.first_entry_word + 2 * e + 1]};
}

// ---- the parsed form: the ONLY place that indexes header words
struct ZpProgram {
    const uint64_t *words = nullptr;
    size_t n_words = 0;
    size_t W = 0, W2 = 0, n_fixed = 0, n_pub = 0, n_chal = 0, n_const = 0, n_instr = 0, K = 0, n_slots = 0, n_s2 = 0, Q = 0;
    const u64 *consts = nullptr, *ins = nullptr, *stage2 = nullptr;       // into the blob
    std::vector<ZpFixedCol> fxc;
    size_t slot_file() const { return n_slots ? n_slots : 1; }      // what an interpreter allocates: a program that announces no slot gets one
    // an operand index of `kind` must be below this -- written once, for the code check and for whoever sizes an operand source
    size_t operand_limit(int kind) const {
        switch (kind) {
            case ZPK_SLOT: return slot_file();
            case ZPK_COL: case ZPK_NEXT: return W + W2;
            case ZPK_FIXED: return n_fixed;
            case ZPK_PUB: return n_pub + n_chal;
            case ZPK_CONST: return n_const;
            case ZPK_XML: return 1;
            default: return 0;
        }
    }
};

// Parse: what every reader does before anything else.  At least twelve words; EVERY count of the header bounded before it enters a sum or sizes
// anything (n_pub + n_chal wraps for a blob that says n_pub = 2^64 - 3, and a public-input entry index is checked against n_pub alone); the sparse
// columns' table entry by entry, and with it the whole-blob length.  The magic is a group below: zp_fixed_columns never looked at it.
inline bool zpi_program_parse(const uint64_t *blob, size_t n_words, ZpProgram *pg, const char **why) {
    *why = "constraint program shorter than its header";
    if (!blob || n_words < ZPH_WORDS) return false;
    pg->words = blob; pg->n_words = n_words;
    pg->W = blob[ZPH_W]; pg->W2 = blob[ZPH_W2]; pg->n_fixed = blob[ZPH_N_FIXED]; pg->n_pub = blob[ZPH_N_PUB]; pg->n_chal = blob[ZPH_N_CHAL];
    pg->n_const = blob[ZPH_N_CONST]; pg->n_instr = blob[ZPH_N_INSTR]; pg->K = blob[ZPH_K]; pg->n_slots = blob[ZPH_N_SLOTS]; pg->n_s2 = blob[ZPH_N_S2];
    pg->Q = blob[ZPH_Q];
    *why = "constraint program length does not match its header";
    if (pg->n_fixed < 2 || pg->n_fixed > 4096 || pg->n_const > (1u << 16) || pg->n_instr > (1u << 24) || pg->n_s2 > (1u << 16) || pg->n_pub > (1u << 24) ||
        pg->n_chal > (1u << 24) || pg->K > (1u << 24))
        return false;
    pg->consts = (const u64 *)blob + ZPH_WORDS; pg->ins = pg->consts + pg->n_const; pg->stage2 = pg->ins + pg->n_instr;
    size_t at = ZPH_WORDS + pg->n_const + pg->n_instr + 4 * pg->n_s2;
    pg->fxc.clear();
    for (size_t k = 2; k < pg->n_fixed; k++) {
        if (at >= n_words) return false;
        const u64 hd = blob[at];
        ZpFixedCol fc{(int)(hd & 0xFF), at + 1, (size_t)(hd >> 8), false};
        if (fc.lp > 32 || fc.n_entries > ((size_t)1 << fc.lp) || at + 1 + 2 * fc.n_entries > n_words) return false;
        for (size_t e = 0; e < fc.n_entries; e++) {
            const ZpFixedEntry en = zpi_fixed_entry(blob, fc, e);
            if (en.pos >= (1ULL << fc.lp) || (en.is_pub ? en.value >= pg->n_pub : en.value >= GL_P)) return false;
            fc.has_pub |= en.is_pub;
        }
        at += 1 + 2 * fc.n_entries;
        pg->fxc.push_back(fc);
    }
    return at == n_words;
}

// Check: named groups; a reader asks for the ones it needs.
enum : unsigned {
    ZPG_MAGIC = 1u << 0,        // the blob starts with "ZPAIR1\0\0"
    ZPG_COUNTS = 1u << 1,       // n_const < 2^16, n_instr < 2^24, n_s2 < 2^16 (the parse admits each limit itself)
    ZPG_N_FIXED = 1u << 2,      // n_fixed < 4096 (the parse admits 4096)
    ZPG_SLOTS_32 = 1u << 3,     // 1 <= n_slots <= 32: the slot file of the row interpreters (64 KiB of LDS)
    ZPG_SLOTS_64K = 1u << 4,    // n_slots <= 2^16 (0 is one slot: ZpProgram::slot_file)
    ZPG_WIDTHS = 1u << 5,       // 1 <= W < 4096, W2 < 4096, K >= 1
    ZPG_QUOTIENT = 1u << 6,     // 1 <= Q <= 16
    ZPG_S2_SHAPE = 1u << 7,     // a stage-2 table exactly when W2 != 0; with a table n_chal == 3
    ZPG_S2_NO_CHAL = 1u << 8,   // without a table n_chal == 0
    ZPG_S2_ENTRIES = 1u << 9,   // every argument of kind 1 or 2, its columns < W, the arguments' widths (3 / 9) sum to W2
    ZPG_CONSTS = 1u << 10,      // every constant < p
    ZPG_CODE = 1u << 11,        // every opcode, every operand against ZpProgram::operand_limit, every destination slot, as many OUTs as K
};
// Who asks for what -- the differences between the readers, as they were when each had its own copy of this code (DESIGN.md "Readers of a
// constraint program").  Every reader parses first; whether a difference is meant is a question for a later change, which edits one line here.
//                                      magic counts n_fixed slots  widths Q  s2: shape no-chal entries  consts code
//   zp_program_eval_ext                  x     .      .      64K     x    .       .      .       .        .      x     (a constant >= p is read mod p)
//   zp_program_fixed_eval_ext (_batch),
//   zp_wrap_aux                          x     .      .      64K     x    .       .      .       .        .      .
//   zp_eval_quotient_rows                x     x      x      32      .    .       .      .       .        x      x
//   zp_fixed_columns (_words)            .     .      .      .       .    .       .      .       .        .      .
//   zp_stark_prove* (make_shape)         x     x      .      .       x    x       x      .       x        .      .     (its quotient stage is zp_eval_quotient_rows)
//   zp_stark_verify* (program_info)      x     .      .      .       x    x       x      x       .        .      .     (its identity is zp_program_eval_ext)
//   zp_stark_check_witness               x     x      x      32      x    x       x      x       x        x      x
constexpr unsigned ZPG_FIXED_EVAL = ZPG_MAGIC | ZPG_SLOTS_64K | ZPG_WIDTHS;
constexpr unsigned ZPG_EVAL_EXT = ZPG_FIXED_EVAL | ZPG_CODE;      // asked in two steps: the code group behind the fixed columns (csrc/verify.hip)
constexpr unsigned ZPG_QUOTIENT_ROWS = ZPG_MAGIC | ZPG_COUNTS | ZPG_N_FIXED | ZPG_SLOTS_32 | ZPG_CONSTS | ZPG_CODE;
constexpr unsigned ZPG_FIXED_COLUMNS = 0;
constexpr unsigned ZPG_PROVE = ZPG_MAGIC | ZPG_COUNTS | ZPG_WIDTHS | ZPG_QUOTIENT | ZPG_S2_SHAPE | ZPG_S2_ENTRIES;
constexpr unsigned ZPG_VERIFY = ZPG_MAGIC | ZPG_WIDTHS | ZPG_QUOTIENT | ZPG_S2_SHAPE | ZPG_S2_NO_CHAL;
constexpr unsigned ZPG_WITNESS = ZPG_QUOTIENT_ROWS | ZPG_PROVE | ZPG_VERIFY;

// the groups of `mask` on a parsed program (every group but the magic); false: *why (may be NULL) names the first refusal
inline bool zpi_program_check(const ZpProgram *pg, unsigned mask, const char **why) {
    const char *dummy;
    const char *&w = why ? *why : dummy;
    w = "constraint program length does not match its header";
    if ((mask & ZPG_COUNTS) && (pg->n_const >= (1u << 16) || pg->n_instr >= (1u << 24) || pg->n_s2 >= (1u << 16))) return false;
    if ((mask & ZPG_N_FIXED) && pg->n_fixed >= 4096) return false;
    w = "constraint program needs more slots than the interpreter has (32)";
    if ((mask & ZPG_SLOTS_32) && (pg->n_slots < 1 || pg->n_slots > 32)) return false;
    if ((mask & ZPG_SLOTS_64K) && pg->n_slots > (1u << 16)) return false;
    w = "program dimensions out of range";
    if ((mask & ZPG_WIDTHS) && (pg->W < 1 || pg->W >= 4096 || pg->W2 >= 4096 || pg->K < 1)) return false;
    if ((mask & ZPG_QUOTIENT) && (pg->Q < 1 || pg->Q > 16)) return false;
    w = "stage-2 table and widths disagree";
    if ((mask & ZPG_S2_SHAPE) && ((pg->n_s2 == 0) != (pg->W2 == 0) || (pg->n_s2 != 0 && pg->n_chal != 3))) return false;
    if ((mask & ZPG_S2_NO_CHAL) && pg->n_s2 == 0 && pg->n_chal != 0) return false;
    if (mask & ZPG_S2_ENTRIES) {
        size_t w2sum = 0;
        for (size_t k = 0; k < pg->n_s2; k++) {
            const u64 *st = pg->stage2 + 4 * k;
            w = "unknown stage-2 argument";
            if (st[0] != ZPS2_PRODUCT && st[0] != ZPS2_LOGUP) return false;
            w = "stage-2 column out of range";
            if (st[1] >= pg->W || st[2] >= pg->W || st[3] >= pg->W) return false;
            w2sum += zpi_stage2_planes(st[0]);
        }
        w = "stage-2 width does not match its table";
        if (w2sum != pg->W2) return false;
    }
    w = "constant not canonical";
    for (size_t i = 0; (mask & ZPG_CONSTS) && i < pg->n_const; i++)
        if (pg->consts[i] >= GL_P) return false;
    if (mask & ZPG_CODE) {
        size_t outs = 0;
        for (size_t i = 0; i < pg->n_instr; i++) {
            const ZpInstr in = zpi_decode(pg->ins[i]);
            w = "unknown opcode in constraint program";
            if (in.op < ZPI_ADD || in.op > ZPI_OUT) return false;
            w = "operand out of range in constraint program";
            for (int o = 0; o < (in.op == ZPI_OUT ? 1 : 2); o++)
                if ((size_t)in.idx[o] >= pg->operand_limit(in.kind[o])) return false;
            w = "destination slot out of range in constraint program";
            if (in.op != ZPI_OUT && (size_t)in.dst >= pg->slot_file()) return false;
            outs += in.op == ZPI_OUT;
        }
        w = "OUT count does not match the header";
        if (outs != pg->K) return false;
    }
    w = "";
    return true;
}
// parse, the magic, then the groups of `mask`
inline bool zpi_program_read(const uint64_t *blob, size_t n_words, unsigned mask, ZpProgram *pg, const char **why) {
    const char *dummy;
    const char *&w = why ? *why : dummy;
    const bool parsed = zpi_program_parse(blob, n_words, pg, &w);
    if ((mask & ZPG_MAGIC) && blob && n_words >= ZPH_WORDS && !zpi_program_magic_ok(blob)) { w = "not a ZPAIR1 constraint program"; return false; }
    return parsed && zpi_program_check(pg, mask, &w);
}

// ---- the walk over a CHECKED program (ZPG_CODE), once.  The reader supplies an environment:
//   typedef ... value;  static value add / sub / mul(value, value);
//   value &slot(int i);               the slot file
//   value load(int kind, int idx);    an operand of any kind (ZPK_SLOT: slot(idx))
//   void out(int k, value v);         constraint k, in program order
// On the device the instruction word is made wave-uniform before it is decoded, so decoding is scalar work and every operand kind a uniform branch;
// the second operand of an OUT is not fetched; the environment inlines completely (nothing goes through memory).
GL_HD u64 zpi_wave_uniform(u64 w) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)w), hi = __builtin_amdgcn_readfirstlane((u32)(w >> 32));
    return ((u64)hi << 32) | lo;
#else
    return w;
#endif
}
template <class Env>
GL_HD void zpi_program_walk(const u64 *ins, int n_instr, Env &env) {
    int k_out = 0;
    for (int i = 0; i < n_instr; i++) {
        const ZpInstr in = zpi_decode(zpi_wave_uniform(ins[i]));       // uniform address: a scalar load on the device
        typename Env::value v[2];
#pragma unroll
        for (int o = 0; o < 2; o++) {
            v[o] = env.load(in.kind[o], in.idx[o]);
            if (in.op == ZPI_OUT) break;
        }
        if (in.op == ZPI_ADD) env.slot(in.dst) = Env::add(v[0], v[1]);
        else if (in.op == ZPI_SUB) env.slot(in.dst) = Env::sub(v[0], v[1]);
        else if (in.op == ZPI_MUL) env.slot(in.dst) = Env::mul(v[0], v[1]);
        else {
            env.out(k_out, v[0]);
            k_out++;
        }
    }
}
