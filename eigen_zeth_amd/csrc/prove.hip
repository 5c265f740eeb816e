// zp_stark_prove: the whole chunk-STARK prover behind ONE C-ABI call -- trace in HBM in, proof bytes out.
// Serves GenChunkProof (proto/prover/v1/prover.proto:56-66; client src/prover/provider.rs:358-390): a host in any
// language binds this entry point and needs neither the Python orchestration (eigen_zeth_amd/stark/prover.py, which stays
// the readable statement of the protocol and the harness of the parity tests) nor a compiler -- the statement is the
// constraint program blob.  Host C++ only: every O(trace) step is one of the library's own entry points (zp_lde,
// zp_merkle_commit, zp_eval_quotient, zp_poly_eval_ext, zp_deep_quotient, zp_fri_fold, ...), the Fiat-Shamir transcript
// runs through zp_poseidon_sponge.  The proof text is byte-identical to proof_to_json(prove(...)) of the Python
// orchestration on the same inputs (tests/test_gpu_native_prover.py), Goldilocks-hash mode.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "sha256.hpp"

namespace {

// The program of a verifier AIR is megabytes (one table entry per scheduled row of every sparse column) and the same blob comes back proof
// after proof: its digest is kept per ctx next to a copy of the blob (compared word for word: a cache hit is a memcmp, not a trust decision).
void program_digest(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, uint8_t dg[32]) { zpi_program_digest_cached(ctx, h_program, program_words, dg); }
}  // namespace
void zpi_program_digest_cached(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, uint8_t dg[32]) {
    if (program_words < (1u << 14)) {                     // small statements: hashing is cheaper than remembering
        Sha256::digest((const uint8_t *)h_program, program_words * 8, dg);
        return;
    }
    for (auto &e : ctx->digest_cache)
        if (e.words.size() == program_words && memcmp(e.words.data(), h_program, program_words * 8) == 0) {
            memcpy(dg, e.dg, 32);
            return;
        }
    Sha256::digest((const uint8_t *)h_program, program_words * 8, dg);
    if (ctx->digest_cache.size() >= 4) ctx->digest_cache.erase(ctx->digest_cache.begin());
    ctx->digest_cache.emplace_back();
    ctx->digest_cache.back().words.assign(h_program, h_program + program_words);
    memcpy(ctx->digest_cache.back().dg, dg, 32);
}
namespace {

// ---- the Fiat-Shamir sponges of stark/transcript.py.  Goldilocks mode: Poseidon-12, rate 8 / capacity 4, on zp_poseidon_sponge.
// BN128 mode: Poseidon-BN254 of width 17 (element 0 = capacity, 1..16 = rate) on zp_poseidon_bn254_sponge; Goldilocks values are
// absorbed three to a field element (every absorb call padded on its own), a Merkle root is one element, and the challenges
// are the three low 64-bit words of the rate elements, each reduced mod p.
struct Transcript {
    zp_ctx *ctx;
    bool bn;
    u64 state[17 * 4];                 // GL: 12 words; BN: 17 elements of 4 words (standard form)
    std::vector<u64> pending, out;     // GL: values; BN: pending holds 4 words per element
    std::vector<u64> log_chal;         // BN: rate element 1 after every flush (4 words each): what the challenge squeezed there is read from (wrap stage B-2)
    std::vector<u64> log_blocks, last_rates, log_caps;   // BN: every absorbed block (16 elements x 4 words) in order; the rate elements of the latest flush; the capacity after every permutation (the wrap circuit's transcript gadgets: zp_wrap_assign)
    int32_t rc = ZP_OK;
    Transcript(zp_ctx *c, bool bn_) : ctx(c), bn(bn_) { memset(state, 0, sizeof state); }
    void absorb(const u64 *v, size_t n) {
        if (!bn) {
            for (size_t i = 0; i < n; i++) pending.push_back(v[i] % GL_P);
        } else {
            for (size_t i = 0; i < n; i += 3) {
                pending.push_back(v[i] % GL_P);
                pending.push_back(i + 1 < n ? v[i + 1] % GL_P : 0);
                pending.push_back(i + 2 < n ? v[i + 2] % GL_P : 0);
                pending.push_back(0);
            }
        }
        out.clear();
    }
    void absorb(const std::vector<u64> &v) { absorb(v.data(), v.size()); }
    void absorb_root(const u64 *root4) {
        if (!bn) { absorb(root4, 4); return; }
        for (int k = 0; k < 4; k++) pending.push_back(root4[k]);
        out.clear();
    }
    void flush(size_t want) {
        const size_t per = bn ? 48 : 8;                    // challenge values one permutation yields
        const size_t extra = want > per ? (want + per - 1) / per - 1 : 0;
        if (!bn) {
            const size_t nblk = (pending.size() + 7) / 8;
            std::vector<u64> blocks(nblk * 8, 0);
            memcpy(blocks.data(), pending.data(), pending.size() * 8);
            pending.clear();
            std::vector<u64> rates((1 + extra) * 8);
            const int32_t r = zp_poseidon_sponge(ctx, (uint64_t *)state, (const uint64_t *)blocks.data(), nblk, extra, (uint64_t *)rates.data());
            if (r != ZP_OK && rc == ZP_OK) rc = r;
            out.assign(rates.begin(), rates.end());
        } else {
            const size_t nel = pending.size() / 4, nblk = (nel + 15) / 16;
            std::vector<u64> blocks(nblk * 64, 0);
            memcpy(blocks.data(), pending.data(), pending.size() * 8);
            pending.clear();
            std::vector<u64> rates((1 + extra) * 64), caps(((nblk ? nblk : 1) + extra) * 4);
            const int32_t r = zp_poseidon_bn254_sponge_caps(ctx, (uint64_t *)state, (const uint64_t *)blocks.data(), nblk, extra, (uint64_t *)rates.data(),
                                                            (uint64_t *)caps.data());
            if (r != ZP_OK && rc == ZP_OK) rc = r;
            log_blocks.insert(log_blocks.end(), blocks.begin(), blocks.end());
            log_caps.insert(log_caps.end(), caps.begin(), caps.end());
            log_chal.insert(log_chal.end(), rates.begin(), rates.begin() + 4);
            last_rates = rates;
            out.clear();
            for (size_t e = 0; e < rates.size() / 4; e++)
                for (int k = 0; k < 3; k++) out.push_back(rates[4 * e + k] % GL_P);
        }
    }
    std::vector<u64> squeeze(size_t n) {
        std::vector<u64> res;
        size_t at = 0;
        while (res.size() < n) {
            if (!pending.empty() || at >= out.size()) {
                flush(n - res.size());
                at = 0;
                if (rc != ZP_OK) { res.resize(n, 0); return res; }
            }
            res.push_back(out[at++]);
        }
        out.erase(out.begin(), out.begin() + at);
        return res;
    }
    e3 challenge() {
        const std::vector<u64> v = squeeze(3);
        return e3_make(v[0], v[1], v[2]);
    }
};

// ---- Merkle trees of the two hash modes behind one set of calls
struct Trees {
    zp_ctx *ctx;
    bool bn;
    static size_t levels16(size_t M) { size_t l = 0; for (size_t n = M; n > 1; n = (n + 15) / 16) l++; return l; }
    size_t tree_words(size_t M) const { return bn ? zp_merkle16_nodes(M) * 4 : (2 * M - 1) * 4; }
    int32_t commit(const u64 *cols, size_t M, int W, u64 *tree) const {
        return bn ? zp_merkle16_commit_bn254(ctx, (const uint64_t *)cols, M, W, (uint64_t *)tree)
                  : zp_merkle_commit(ctx, (const uint64_t *)cols, M, W, (uint64_t *)tree);
    }
    int32_t root(const u64 *tree, size_t M, u64 *out4) const {
        return zp_d2h(ctx, out4, tree + tree_words(M) - 4, 32);           // both layouts end with the root
    }
    size_t path_words(size_t M) const {          // per query
        if (bn) return levels16(M) * 64;
        size_t d = 0;
        while (((size_t)1 << d) < M) d++;
        return (d ? d : 1) * 4;
    }
    int32_t open(const u64 *tree, size_t M, const u64 *idx, int nq, u64 *out) const {
        return bn ? zp_merkle16_open_batch_bn254(ctx, (const uint64_t *)tree, M, (const uint64_t *)idx, nq, (uint64_t *)out)
                  : zp_merkle_open_batch(ctx, (const uint64_t *)tree, M, (const uint64_t *)idx, nq, (uint64_t *)out);
    }
};

// what a prover opened in one tree at the query indices: per query `width` values (one leaf) and `pw` path words, the tree over `rows` leaves
struct Opened {
    std::vector<u64> vals, paths;
    size_t width = 0, rows = 0, pw = 0;
    void shape(size_t nq, size_t width_, size_t rows_, size_t pw_) {
        width = width_; rows = rows_; pw = pw_;
        vals.resize(nq * width);
        paths.resize(nq * pw);
    }
};

// the binary openings record of a BN128-mode proof (zp_stark_openings documents the layout), kept on the ctx.  trees: trace, quotient,
// [stage 2], FRI layers
struct TreeOut { const u64 *root; const Opened *o; };
void openings_record(zp_ctx *ctx, const Transcript &tr, const std::vector<u64> &qidx, int logm, const std::vector<TreeOut> &trees) {
    std::vector<u64> &rec = ctx->last_openings;
    rec.clear();
    rec.insert(rec.end(), {0x33304e45504f5a50ULL /* "PZOPEN03" */, (u64)qidx.size(), (u64)trees.size(), (u64)logm});
    for (const TreeOut &t : trees) rec.insert(rec.end(), {(u64)t.o->width, (u64)t.o->rows, (u64)Trees::levels16(t.o->rows)});
    for (const TreeOut &t : trees) rec.insert(rec.end(), t.root, t.root + 4);
    for (size_t i = 0; i < qidx.size(); i++) {
        rec.push_back(qidx[i]);
        for (const TreeOut &t : trees) {
            rec.insert(rec.end(), t.o->vals.begin() + i * t.o->width, t.o->vals.begin() + (i + 1) * t.o->width);
            rec.insert(rec.end(), t.o->paths.begin() + i * t.o->pw, t.o->paths.begin() + (i + 1) * t.o->pw);
        }
    }
    // the transcript (round 5: the wrap circuit hashes it too): every absorbed block, then the rate elements the indices were read from
    rec.push_back((u64)(tr.log_blocks.size() / 64));
    rec.push_back((u64)(tr.last_rates.size() / 64));
    rec.insert(rec.end(), tr.log_blocks.begin(), tr.log_blocks.end());
    rec.insert(rec.end(), tr.last_rates.begin(), tr.last_rates.end());
    rec.insert(rec.end(), tr.log_caps.begin(), tr.log_caps.end());         // one per permutation: n_blocks + (n_rates - 1)
    rec.push_back((u64)(tr.log_chal.size() / 4));                           // the rate element behind every challenge, in squeeze order
    rec.insert(rec.end(), tr.log_chal.begin(), tr.log_chal.end());
}

// Device buffers of one proof.  They come from, and go back to, a per-ctx pool keyed by size: everything runs on the ctx
// stream, so a buffer handed out again is only touched by work enqueued after its previous user.
#define PROVE_POOL_CAP ((size_t)8 << 30)    /* per ctx: a 2^20 x 76 proof keeps ~3 GiB; 8 proving ctxs share one 288 GB GPU */
struct DevBufs {
    zp_ctx *ctx;
    std::vector<std::pair<void *, size_t>> bufs;
    explicit DevBufs(zp_ctx *c) : ctx(c) {}
    ~DevBufs() { for (auto &b : bufs) give_back(b.first, b.second); }
    void give_back(void *p, size_t bytes) {
        if (ctx->prove_pool_bytes + bytes <= PROVE_POOL_CAP) {
            ctx->prove_pool.emplace(bytes, p);
            ctx->prove_pool_bytes += bytes;
        } else {
            (void)zp_dev_free(ctx, p);
        }
    }
    int32_t alloc(size_t elems, u64 **out) {
        const size_t bytes = (elems ? elems : 1) * 8;
        auto it = ctx->prove_pool.find(bytes);
        void *p = nullptr;
        if (it != ctx->prove_pool.end()) {
            p = it->second;
            ctx->prove_pool.erase(it);
            ctx->prove_pool_bytes -= bytes;
        } else {
            int32_t r = zp_dev_alloc(ctx, bytes, &p);
            if (r == ZP_ERR_NOMEM && !ctx->prove_pool.empty()) {      // give the pool back to the device and try once more
                for (auto &kv : ctx->prove_pool) (void)zp_dev_free(ctx, kv.second);
                ctx->prove_pool.clear();
                ctx->prove_pool_bytes = 0;
                r = zp_dev_alloc(ctx, bytes, &p);
            }
            if (r != ZP_OK) return r;
        }
        bufs.emplace_back(p, bytes);
        *out = (u64 *)p;
        return ZP_OK;
    }
    void release(u64 *p) {
        for (size_t i = 0; i < bufs.size(); i++)
            if (bufs[i].first == (void *)p) { give_back(bufs[i].first, bufs[i].second); bufs.erase(bufs.begin() + i); return; }
    }
    void forget(u64 *p) {      // ownership moves elsewhere (a ctx-level cache)
        for (size_t i = 0; i < bufs.size(); i++)
            if (bufs[i].first == (void *)p) { bufs.erase(bufs.begin() + i); return; }
    }
};

// ---- JSON text exactly as json.dumps(proof, separators=(",", ":")) writes it
// a chunk proof's text is ~150 000 decimal numbers: two digits per division from a table instead of snprintf (6.4 -> ~2 ms of a 90 ms proof at 2^22 rows)
void j_u64(std::string &s, u64 v) {
    static const char D2[201] =
        "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869"
        "707172737475767778798081828384858687888990919293949596979899";
    char b[24];
    int at = 24;
    while (v >= 100) {
        const unsigned r = (unsigned)(v % 100);
        v /= 100;
        b[--at] = D2[2 * r + 1];
        b[--at] = D2[2 * r];
    }
    if (v >= 10) {
        b[--at] = D2[2 * v + 1];
        b[--at] = D2[2 * v];
    } else {
        b[--at] = (char)('0' + v);
    }
    s.append(b + at, (size_t)(24 - at));
}
void j_list(std::string &s, const u64 *v, size_t n) {
    s += '[';
    for (size_t i = 0; i < n; i++) { if (i) s += ','; j_u64(s, v[i]); }
    s += ']';
}
void j_e3list(std::string &s, const std::vector<u64> &v) {   // [[a,b,c],...]
    s += '[';
    for (size_t i = 0; i * 3 < v.size(); i++) { if (i) s += ','; j_list(s, &v[3 * i], 3); }
    s += ']';
}
void j_dec256(std::string &s, const u64 *w4) {     // "decimal" of a 256-bit little-endian value, quoted
    // 19 digits at a time (10^19 < 2^64): five long divisions instead of 78 -- a BN128-mode proof text carries ~20 000 such numbers
    // (16 digests per level of every authentication path), and digit-by-digit they were 8 ms of a 93 ms final STARK
    constexpr u64 TEN19 = 10000000000000000000ULL;
    u64 v[4] = {w4[0], w4[1], w4[2], w4[3]};
    u64 chunk[5];
    int n = 0;
    while (v[0] | v[1] | v[2] | v[3]) {
        unsigned __int128 rem = 0;
        for (int k = 3; k >= 0; k--) {
            const unsigned __int128 cur = (rem << 64) | v[k];
            v[k] = (u64)(cur / TEN19);
            rem = cur % TEN19;
        }
        chunk[n++] = (u64)rem;
    }
    s += '"';
    if (!n) {
        s += '0';
    } else {
        char b[24];
        snprintf(b, sizeof b, "%llu", (unsigned long long)chunk[n - 1]);
        s += b;
        for (int k = n - 2; k >= 0; k--) {
            snprintf(b, sizeof b, "%019llu", (unsigned long long)chunk[k]);
            s += b;
        }
    }
    s += '"';
}
void j_root(std::string &s, const u64 *root4, bool bn) {
    if (!bn) { j_list(s, root4, 4); return; }
    s += '[';
    j_dec256(s, root4);
    s += ']';
}
void j_opening_bn(std::string &s, const u64 *vals, size_t W, const u64 *path, size_t levels) {   // path: per level 16 digests as strings
    s += "{\"values\":";
    j_list(s, vals, W);
    s += ",\"path\":[";
    for (size_t l = 0; l < levels; l++) {
        if (l) s += ',';
        s += '[';
        for (int c = 0; c < 16; c++) { if (c) s += ','; j_dec256(s, path + (l * 16 + c) * 4); }
        s += ']';
    }
    s += "]}";
}
void j_opening(std::string &s, const u64 *vals, size_t W, const u64 *path, size_t depth) {   // {"values":[..],"path":[[4]..]}
    s += "{\"values\":";
    j_list(s, vals, W);
    s += ",\"path\":[";
    for (size_t d = 0; d < depth; d++) { if (d) s += ','; j_list(s, path + 4 * d, 4); }
    s += "]}";
}

#define PV_TRY(expr)                                                    \
    do {                                                                \
        const int32_t rc_ = (expr);                                     \
        if (rc_ != ZP_OK) return rc_;                                   \
    } while (0)

// ======================================================================================================================
// The steps of the protocol that the single-device prover (prove_impl) and the sharded one (prove_sharded_impl) share: what defines the
// transcript and the proof text exists once.  A step works on the ctx stream with the DevBufs of its caller and never touches a communicator.

// the arguments of the four entry points (pow_bits = 0 in BN128 mode; the sharded ones pass this rank's columns as d_trace)
struct ProveArgs {
    const char *air_name;
    const uint64_t *h_program;
    size_t program_words;
    const uint64_t *d_trace;
    size_t trace_words;
    const uint64_t *h_pubs;
    int32_t n_pubs, logn, logb, fri_logf, fri_final_log, n_queries, pow_bits;
    char **out_json;
    size_t *out_len;
};

// measurement aid (ZP_PROVE_TRACE=1): host-clock milliseconds since entry at the stage boundaries, the stream drained at each -- where the
// wall time of a proof goes that the per-entry-point GPU times do not show.  The shared steps mark their own end.
struct StageClock {
    zp_ctx *ctx;
    const char *air_name;
    int logn;
    std::chrono::steady_clock::time_point t_entry;
    void operator()(const char *what) const {
        static const bool trace_on = getenv("ZP_PROVE_TRACE") != nullptr;
        if (!trace_on) return;
        (void)hipStreamSynchronize(ctx->stream);
        fprintf(stderr, "[prove %s 2^%d] %-28s %8.3f ms\n", air_name, logn, what,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count());
    }
};

// ... validated, with what the provers read from the program header and derive from the parameters
struct Shape : ProveArgs {
    ZpProgram pg;                      // the parsed program: W, W2, K, Q, n_s2, stage2 (n_s2 x (kind, three trace columns)), fxc
    bool bn;
    size_t Wt;                         // pg.W + pg.W2
    int logm;
    size_t N, M;
    u64 shift, root32, wN;
    uint8_t dg[32];                    // AIR digest: sha256 of the blob; the first 16 hex digits name it, four little-endian words go into the transcript
    char dg_hex[17];
    StageClock mark;
    // BN128 mode: a leaf holds 2^g rows i, i + M', ... of its tree (the column-major matrix reinterpreted as [width 2^g][M'], like a
    // FRI layer), g the largest with width 2^g <= 56 values = one width-17 permutation per leaf (stark/prover.py:
    // bn128_rows_per_leaf_log; Goldilocks mode: g = 0)
    int rows_per_leaf_log(size_t width) const {
        int g = 0;
        if (bn && width)
            while ((width << (g + 1)) <= 56 && g + 1 <= logm - 4) g++;
        return g;
    }
};

// everything both provers require of their arguments (d_trace and trace_words depend on who holds the columns: the provers check them)
int32_t make_shape(zp_ctx *ctx, bool bn, const ProveArgs &a, Shape *sh) {
    ZP_ARG(ctx, a.air_name && a.h_program && a.out_json && a.out_len && (a.h_pubs || a.n_pubs == 0), "null pointer");
    {   // the name goes into the proof text verbatim: letters, digits, '_', '-', '.' only
        const size_t nl = strlen(a.air_name);
        bool ok = nl >= 1 && nl <= 64;
        for (size_t i = 0; ok && i < nl; i++) {
            const char ch = a.air_name[i];
            ok = (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '-' || ch == '.';
        }
        ZP_ARG(ctx, ok, "air_name must be 1..64 characters of [A-Za-z0-9_.-]");
    }
    const char *why;
    ZP_ARG(ctx, zpi_program_read(a.h_program, a.program_words, ZPG_PROVE, &sh->pg, &why), why);
    ZP_ARG(ctx, (size_t)a.n_pubs == sh->pg.n_pub, "number of public inputs does not match the program");
    ZP_ARG(ctx, a.logn >= 1 && a.logb >= 1 && a.logn + a.logb <= 30 && a.fri_logf >= 1 && a.fri_logf <= 4 && a.fri_final_log >= 0 &&
                    a.fri_final_log < a.logn && a.n_queries >= 1 && a.n_queries <= 4096 && a.pow_bits >= 0 && a.pow_bits <= 40,
           "STARK parameters out of range");
    ZP_ARG(ctx, sh->pg.Q <= ((size_t)1 << a.logb), "the blow-up must cover the quotient degree");
    for (int i = 0; i < a.n_pubs; i++) ZP_ARG(ctx, a.h_pubs[i] < GL_P, "public input not canonical");

    static_cast<ProveArgs &>(*sh) = a;
    sh->bn = bn;
    sh->Wt = sh->pg.W + sh->pg.W2;
    sh->logm = a.logn + a.logb; sh->N = (size_t)1 << a.logn; sh->M = (size_t)1 << sh->logm;
    sh->shift = ctx->coset_shift; sh->root32 = ctx->root32; sh->wN = gl_root(sh->root32, a.logn);
    program_digest(ctx, a.h_program, a.program_words, sh->dg);
    for (int i = 0; i < 8; i++) snprintf(sh->dg_hex + 2 * i, 3, "%02x", sh->dg[i]);
    sh->mark = StageClock{ctx, a.air_name, a.logn, std::chrono::steady_clock::now()};
    return ZP_OK;
}

// the first block of the transcript: parameters, domain, AIR digest, public inputs
int32_t transcript_head(zp_ctx *ctx, const Shape &sh, Transcript &tr, const Trees &T, DevBufs &dev) {
    std::vector<u64> first = {(u64)sh.logn, (u64)sh.logb, (u64)sh.pg.W, (u64)sh.pg.W2, (u64)sh.fri_logf, (u64)sh.fri_final_log, (u64)sh.n_queries, (u64)sh.pow_bits,
                              sh.root32, sh.shift};
    for (int i = 0; i < 4; i++) {
        u64 wd = 0;
        for (int k = 0; k < 8; k++) wd |= (u64)sh.dg[8 * i + k] << (8 * k);
        first.push_back(wd % GL_P);
    }
    first.push_back((u64)sh.n_pubs);
    if (sh.n_pubs <= 64) {
        for (int i = 0; i < sh.n_pubs; i++) first.push_back(sh.h_pubs[i]);
        tr.absorb(first);
        sh.mark("transcript head");
        return ZP_OK;
    }
    // a long public-input vector (a verifier AIR: every root, index and opened value of its inner proofs) enters the transcript
    // as ONE commitment instead of thousands of dependent sponge permutations: Goldilocks mode: rows of 8 values (zero padded,
    // row count a power of two >= 2), binary Poseidon tree;  BN128 mode: rows of 48 values, column-major, 16-ary tree
    // (the sharded prover too, replicated: a few thousand permutations at most)
    tr.absorb(first);
    size_t Mp;
    std::vector<u64> mat;
    if (!sh.bn) {
        Mp = 2;
        while (Mp * 8 < (size_t)sh.n_pubs) Mp <<= 1;
        mat.assign(Mp * 8, 0);
        for (int i = 0; i < sh.n_pubs; i++) mat[i] = sh.h_pubs[i];
    } else {
        Mp = ((size_t)sh.n_pubs + 47) / 48;
        mat.assign(Mp * 48, 0);
        for (int i = 0; i < sh.n_pubs; i++) mat[(size_t)(i % 48) * Mp + (size_t)(i / 48)] = sh.h_pubs[i];
    }
    u64 *dmat, *dtree;
    PV_TRY(dev.alloc(mat.size(), &dmat));
    PV_TRY(dev.alloc(T.tree_words(Mp), &dtree));
    PV_TRY(zp_h2d(ctx, dmat, mat.data(), mat.size() * 8));
    if (!sh.bn) PV_TRY(zp_merkle_commit_rows(ctx, (const uint64_t *)dmat, Mp, 8, (uint64_t *)dtree));
    else PV_TRY(T.commit(dmat, Mp, 48, dtree));
    u64 rootp[4];
    PV_TRY(T.root(dtree, Mp, rootp));
    dev.release(dmat);
    dev.release(dtree);
    tr.absorb_root(rootp);
    sh.mark("transcript head");
    return ZP_OK;
}

// The fixed columns of a program on its evaluation domain (zp_fixed_columns: boundary selectors + one extended period of every sparse periodic
// column), from the ctx's cache: they depend on the domain and the program only; columns that hold public inputs (expected roots / indices /
// transcript words of a verifier AIR: 37 of 104 at the service's size) are refreshed in place per proof, the others stay.  The buffer belongs
// to the ctx.  (Both provers: the sharded one cuts its row windows out of it.)
int32_t fixed_columns_cached(zp_ctx *ctx, const Shape &sh, u64 **out) {
    bool has_pub = false;
    for (const ZpFixedCol &fc : sh.pg.fxc) has_pub |= fc.has_pub;
    const size_t fwords = zp_fixed_columns_words(sh.h_program, sh.program_words, sh.logn, sh.logb);
    ZP_ARG(ctx, fwords != 0, "fixed column longer than the trace");
    char key[128];
    snprintf(key, sizeof key, "%d/%d/%llx/%llx/%s", sh.logn, sh.logb, (unsigned long long)sh.shift, (unsigned long long)sh.root32, sh.pg.fxc.empty() ? "" : sh.dg_hex);
    auto it = ctx->prove_fixed.find(key);
    if (it != ctx->prove_fixed.end()) {
        *out = it->second;
        if (has_pub) {
            ZpStage stage_fx(ctx, "fixed_columns");
            PV_TRY(zpi_fixed_columns_build(ctx, sh.h_program, sh.program_words, sh.h_pubs, sh.n_pubs, sh.logn, sh.logb, sh.shift, (uint64_t *)*out, fwords, true));
        }
        return ZP_OK;
    }
    // (a verifier AIR's columns are gigabytes -- 91 full-length columns at the service's size: 3 GB --; a ctx that has met many shapes
    // starts over rather than grow without bound)
    if (ctx->prove_fixed_bytes + fwords * 8 > ((size_t)24 << 30) && !ctx->prove_fixed.empty()) {
        PV_TRY(zp_sync(ctx));
        for (auto &kv : ctx->prove_fixed) (void)hipFree(kv.second);
        ctx->prove_fixed.clear();
        ctx->prove_fixed_bytes = 0;
    }
    void *pf = nullptr;
    PV_TRY(zp_dev_alloc(ctx, fwords * 8, &pf));
    const int32_t r = zp_fixed_columns(ctx, sh.h_program, sh.program_words, sh.h_pubs, sh.n_pubs, sh.logn, sh.logb, sh.shift, (uint64_t *)pf, fwords);
    if (r != ZP_OK) { (void)zp_dev_free(ctx, pf); return r; }
    ctx->prove_fixed[key] = (u64 *)pf;
    ctx->prove_fixed_bytes += fwords * 8;
    *out = (u64 *)pf;
    return ZP_OK;
}

// Generated constraint kernels (AIR plug-in ABI: stark/air.py writes them) are kept per ctx under the 64 hex digits of the program's
// digest: form "" = the whole-domain kernel (`zpair_<air>_quotient`), form "rows:" = its row-window form (`zpair_<air>_quotient_rows`), form
// "witness:" = the constraint check on the trace domain (`zpair_<air>_quotient_witness`, run by csrc/witness_check.hip)
typedef int (*zp_air_quotient_fn)(void *stream, const u64 *cols, const u64 *fixedc, u64 M, u64 b, const u64 *pub, const u64 *apow, const u64 *zhinv,
                                  const u64 *xs_lo, const u64 *xs_hi, int lb, u64 shift, u64 wlast, u64 *out);
typedef int (*zp_air_quotient_rows_fn)(void *stream, const u64 *cols, u64 sc, const u64 *fixedc, u64 sf, u64 M, u64 b, u64 row0, u64 nrows, const u64 *pub,
                                       const u64 *apow, const u64 *zhinv, const u64 *xs_lo, const u64 *xs_hi, int lb, u64 shift, u64 wlast, u64 *out, u64 so);
std::string air_kernel_key(const char *form, const uint8_t dg[32]) { return zpi_air_kernel_key(form, dg); }
}  // namespace
std::string zpi_air_kernel_key(const char *form, const uint8_t dg[32]) {
    char hex[65];
    for (int i = 0; i < 32; i++) snprintf(hex + 2 * i, 3, "%02x", dg[i]);
    return std::string(form) + std::string(hex, 64);
}
namespace {
int32_t set_air_kernel(zp_ctx *ctx, const char *form, const uint64_t *h_program, size_t program_words, void *fn) {
    if (!ctx) return ZP_ERR_ARG;
    ZP_ARG(ctx, h_program && program_words >= 8 && program_words < ((size_t)1 << 28), "null / implausible program");
    try {
        uint8_t dg[32];
        Sha256::digest((const uint8_t *)h_program, program_words * 8, dg);
        const std::string k = air_kernel_key(form, dg);
        if (fn) ctx->air_kernels[k] = fn;
        else ctx->air_kernels.erase(k);
    } catch (...) {
        ctx->err = "out of host memory";
        return ZP_ERR_NOMEM;
    }
    return ZP_OK;
}

// the small operands of the constraint quotient: powers of alpha and 1 / Z_H (host; what the interpreter takes), and, when a generated
// kernel of this program is registered under `form`, that kernel with its operands on the device
struct QuotientOps {
    std::vector<u64> apow, zhinv;      // alpha^k, k < K (3 words each); 1 / Z_H on the 2^logb cosets of the trace domain
    void *plug = nullptr;              // the generated kernel, or none: the interpreter runs.  With a kernel:
    u64 *d_ops = nullptr;              // ONE device buffer [pub | 0 | apow | zhinv] from the caller's DevBufs (the caller releases it)
    size_t o_ap = 0, o_zh = 0;         // where apow and zhinv start in it
    const uint64_t *xlo = nullptr, *xhi = nullptr;      // zp_domain_tables
    int32_t xlb = 0;
};
int32_t quotient_operands(zp_ctx *ctx, const Shape &sh, const char *form, const e3 &alpha, const std::vector<u64> &pubchal, DevBufs &dev, QuotientOps *q) {
    q->apow.resize(3 * sh.pg.K);
    e3 cur = e3_make(1, 0, 0);
    for (size_t k = 0; k < sh.pg.K; k++) { memcpy(&q->apow[3 * k], cur.c, 24); cur = e3_mul(cur, alpha); }
    q->zhinv.resize((size_t)1 << sh.logb);
    const u64 sN = gl_pow(sh.shift, (u64)sh.N), wb = gl_root(sh.root32, sh.logb);
    u64 p = 1;
    for (size_t j = 0; j < q->zhinv.size(); j++) { q->zhinv[j] = gl_inv(gl_sub(gl_mul(sN, p), 1)); p = gl_mul(p, wb); }
    if (ctx->air_kernels.empty()) return ZP_OK;
    // (the digest of the Shape -- through the per-ctx cache, a memcmp for a program seen before -- not a second SHA-256 of the blob: for a
    // verifier AIR's 7 MB that second hash was 16 ms of every recursion STARK, round 5.  Since that round the generated kernels read the
    // sparse periodic fixed columns too -- one extended period each, zp_fixed_columns' layout)
    auto it = ctx->air_kernels.find(air_kernel_key(form, sh.dg));
    if (it == ctx->air_kernels.end()) return ZP_OK;
    q->plug = it->second;
    std::vector<u64> ops(pubchal);
    ops.push_back(0);
    q->o_ap = ops.size();
    ops.insert(ops.end(), q->apow.begin(), q->apow.end());
    q->o_zh = ops.size();
    ops.insert(ops.end(), q->zhinv.begin(), q->zhinv.end());
    PV_TRY(dev.alloc(ops.size(), &q->d_ops));
    PV_TRY(zp_h2d(ctx, q->d_ops, ops.data(), ops.size() * 8));
    return zp_domain_tables(ctx, sh.logm, &q->xlo, &q->xhi, &q->xlb);
}

// Q > 1: q(x) = sum_j (x / shift)^(jN) qt_j(x): the pieces are slices of the coefficient vector of q(shift X) (c_i shift^i); their LDEs
// (*pext: u64[3 Q][M]) get committed.  (Q == 1: the quotient is committed as it stands and never leaves the evaluation form.)  Ends with
// the forward transform ENQUEUED: the caller synchronises before it releases *dqcoef and *pad, its own way
int32_t split_quotient(zp_ctx *ctx, const Shape &sh, DevBufs &dev, const u64 *dq, u64 **dqcoef, u64 **pad, u64 **pext) {
    const size_t Q = sh.pg.Q, N = sh.N, M = sh.M;
    PV_TRY(dev.alloc(3 * M, dqcoef));
    PV_TRY(zp_intt(ctx, (const uint64_t *)dq, (uint64_t *)*dqcoef, sh.logm, 3));
    PV_TRY(dev.alloc(3 * Q * M, pad));
    PV_TRY(zp_dev_zero(ctx, *pad, 3 * Q * M * 8));
    for (size_t j = 0; j < Q; j++)
        for (int c = 0; c < 3; c++) PV_TRY(zp_d2d(ctx, *pad + (3 * j + c) * M, *dqcoef + c * M + j * N, N * 8));
    PV_TRY(dev.alloc(3 * Q * M, pext));
    return zp_ntt(ctx, (const uint64_t *)*pad, (uint64_t *)*pext, sh.logm, (int32_t)(3 * Q));
}

// FRI over the DEEP quotient df (u64[3][M], whole on the device): commit a layer, fold it with the challenge its root yields, until the
// final layer, which enters the transcript in the clear
struct FriLayer { int lg, f; u64 *tree, *data; u64 root[4]; };
struct Fri {
    std::vector<FriLayer> layers;
    std::vector<u64> final_l;          // u64[3][2^final_log]
    int final_log;
};
int32_t fri_commit(zp_ctx *ctx, const Shape &sh, Transcript &tr, const Trees &T, DevBufs &dev, u64 *df, Fri *fri) {
    const int stop = sh.fri_final_log + sh.logb;
    int cur = sh.logm;
    u64 cur_shift = sh.shift;
    u64 *dlayer = df;
    while (cur > stop) {
        const int f = sh.fri_logf < cur - stop ? sh.fri_logf : cur - stop;
        FriLayer L;
        L.lg = cur; L.f = f; L.data = dlayer;
        const size_t m = (size_t)1 << (cur - f);
        PV_TRY(dev.alloc(T.tree_words(m), &L.tree));
        PV_TRY(T.commit(dlayer, m, 3 << f, L.tree));   // leaf = the 2^f * 3 values folded together
        PV_TRY(T.root(L.tree, m, L.root));
        tr.absorb_root(L.root);
        const e3 beta = tr.challenge();
        PV_TRY(tr.rc);
        u64 *next;
        PV_TRY(dev.alloc((size_t)3 << (cur - f), &next));
        PV_TRY(zp_fri_fold(ctx, (const uint64_t *)dlayer, (uint64_t *)next, cur, f, (const uint64_t *)beta.c, cur_shift));
        fri->layers.push_back(L);
        dlayer = next;
        cur_shift = gl_pow(cur_shift, (u64)1 << f);
        cur -= f;
    }
    fri->final_log = cur;
    fri->final_l.resize((size_t)3 << cur);
    PV_TRY(zp_d2h(ctx, fri->final_l.data(), dlayer, fri->final_l.size() * 8));
    for (int c = 0; c < 3; c++) tr.absorb(&fri->final_l[(size_t)c << cur], (size_t)1 << cur);   // plane by plane (BN128 mode pads every call)
    sh.mark("DEEP + FRI");
    return ZP_OK;
}

// proof of work, then the query indices (rows of the 2^logm-point domain)
int32_t grind_and_indices(zp_ctx *ctx, const Shape &sh, Transcript &tr, u64 *nonce, std::vector<u64> *qidx) {
    *nonce = 0;
    if (sh.pow_bits) {
        const std::vector<u64> seed = tr.squeeze(4);
        PV_TRY(tr.rc);
        PV_TRY(zp_pow_grind(ctx, (const uint64_t *)seed.data(), sh.pow_bits, (uint64_t *)nonce));
        tr.absorb(nonce, 1);
    }
    *qidx = tr.squeeze((size_t)sh.n_queries);
    PV_TRY(tr.rc);
    for (u64 &v : *qidx) v &= (sh.M - 1);
    return ZP_OK;
}

// open a tree that is whole on this device at the queries: leaf i of `rows` leaves = row i of mat u64[width][rows]
int32_t open_tree(zp_ctx *ctx, const Trees &T, const u64 *mat, const u64 *tree, size_t rows, size_t width, const std::vector<u64> &qidx, Opened *o) {
    std::vector<u64> idx = qidx;
    for (u64 &v : idx) v &= (rows - 1);
    o->shape(qidx.size(), width, rows, T.path_words(rows));
    PV_TRY(zp_gather_rows(ctx, (const uint64_t *)mat, rows, (int32_t)width, (const uint64_t *)idx.data(), (int32_t)qidx.size(), (uint64_t *)o->vals.data()));
    return T.open(tree, rows, idx.data(), (int)qidx.size(), o->paths.data());
}
int32_t fri_open(zp_ctx *ctx, const Shape &sh, const Trees &T, const Fri &fri, const std::vector<u64> &qidx, std::vector<Opened> *fo) {
    fo->resize(fri.layers.size());
    for (size_t li = 0; li < fri.layers.size(); li++) {
        const FriLayer &L = fri.layers[li];
        PV_TRY(open_tree(ctx, T, L.data, L.tree, (size_t)1 << (L.lg - L.f), (size_t)3 << L.f, qidx, &(*fo)[li]));
    }
    sh.mark("queries opened");
    return ZP_OK;
}

// what a proof says besides its header; the provers differ in how they came by it, not in how it is written down
struct ProofBody {
    const u64 *root1, *rootq, *root2;                  // root2, stage2: read when the program has stage-2 arguments
    const std::vector<u64> &ev_all, &ev_next;
    const Fri &fri;
    u64 nonce;
    const std::vector<u64> &qidx;
    const Opened &trace, &quotient, &stage2;
    const std::vector<Opened> &fo;
};
// the openings record (BN128 mode), the text, and its hand-over to the caller
int32_t write_proof(zp_ctx *ctx, const Shape &sh, const Transcript &tr, const ProofBody &p) {
    const bool bn = sh.bn;
    const size_t nl = p.fri.layers.size();
    if (bn) {       // the same openings in binary, for the Groth16 wrap's witness (zp_stark_openings -> zp_wrap_assign): no text round trip
        std::vector<TreeOut> trees = {{p.root1, &p.trace}, {p.rootq, &p.quotient}};
        if (sh.pg.n_s2) trees.push_back({p.root2, &p.stage2});
        for (size_t li = 0; li < nl; li++) trees.push_back({p.fri.layers[li].root, &p.fo[li]});
        openings_record(ctx, tr, p.qidx, sh.logm, trees);
    }
    std::string s;
    s.reserve(p.qidx.size() * (sh.Wt + 3 * sh.pg.Q + 64) * 24 + (1 << 16));
    s += "{\"air\":\"";
    s += sh.air_name;
    s += "\",\"air_digest\":\"";
    s += sh.dg_hex;
    s += "\",\"params\":{\"logn\":";
    j_u64(s, (u64)sh.logn); s += ",\"logb\":"; j_u64(s, (u64)sh.logb); s += ",\"fri_logf\":"; j_u64(s, (u64)sh.fri_logf);
    s += ",\"fri_final_log\":"; j_u64(s, (u64)sh.fri_final_log); s += ",\"n_queries\":"; j_u64(s, (u64)sh.n_queries);
    s += ",\"pow_bits\":"; j_u64(s, (u64)sh.pow_bits);
    if (bn) s += ",\"hash\":\"bn128\"";
    s += "},\"root32\":"; j_u64(s, sh.root32);
    s += ",\"shift\":"; j_u64(s, sh.shift);
    s += ",\"publics\":"; j_list(s, (const u64 *)sh.h_pubs, (size_t)sh.n_pubs);
    s += ",\"roots\":{\"trace\":"; j_root(s, p.root1, bn);
    s += ",\"quotient\":"; j_root(s, p.rootq, bn);
    if (sh.pg.n_s2) { s += ",\"stage2\":"; j_root(s, p.root2, bn); }
    s += "},\"evals\":{\"z\":"; j_e3list(s, p.ev_all);
    s += ",\"zw\":"; j_e3list(s, p.ev_next);
    s += "},\"fri\":{\"roots\":[";
    for (size_t li = 0; li < nl; li++) { if (li) s += ','; j_root(s, p.fri.layers[li].root, bn); }
    s += "],\"final\":[";
    for (int c = 0; c < 3; c++) { if (c) s += ','; j_list(s, &p.fri.final_l[(size_t)c << p.fri.final_log], (size_t)1 << p.fri.final_log); }
    s += "]},\"queries\":[";
    for (size_t i = 0; i < p.qidx.size(); i++) {
        if (i) s += ',';
        s += "{\"index\":"; j_u64(s, p.qidx[i]);
        auto opening = [&](const Opened &o) {      // a binary tree's path has one digest per level: log2(rows) of them
            size_t depth = 0;
            while (((size_t)1 << depth) < o.rows) depth++;
            if (bn) j_opening_bn(s, &o.vals[i * o.width], o.width, &o.paths[i * o.pw], Trees::levels16(o.rows));
            else j_opening(s, &o.vals[i * o.width], o.width, &o.paths[i * o.pw], depth);
        };
        s += ",\"trace\":"; opening(p.trace);
        s += ",\"quotient\":"; opening(p.quotient);
        if (sh.pg.n_s2) { s += ",\"stage2\":"; opening(p.stage2); }
        s += ",\"fri\":[";
        for (size_t li = 0; li < nl; li++) { if (li) s += ','; opening(p.fo[li]); }
        s += "]}";
    }
    s += ']';
    if (sh.pow_bits) { s += ",\"pow_nonce\":"; j_u64(s, p.nonce); }
    s += '}';
    sh.mark("proof text");
    char *buf = (char *)malloc(s.size() + 1);
    if (!buf) { ctx->err = "out of host memory for the proof text"; return ZP_ERR_NOMEM; }
    memcpy(buf, s.data(), s.size() + 1);
    *sh.out_json = buf;
    *sh.out_len = s.size();
    return ZP_OK;
}

// no C++ exception may cross the C ABI (a Rust or ctypes caller cannot unwind it): allocation failures of the host-side vectors /
// strings (sizes follow caller parameters: n_queries * path words, 3 << fri_final_log, ...) come back as error codes
template <class Body>
int32_t guarded(zp_ctx *ctx, Body body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try { ctx->err = "out of host memory while building the proof"; } catch (...) {}
        return ZP_ERR_NOMEM;
    } catch (const std::exception &e) {
        try { ctx->err = std::string("internal error: ") + e.what(); } catch (...) {}
        return ZP_ERR_INTERNAL;
    } catch (...) {
        return ZP_ERR_INTERNAL;
    }
}

// ---- "prove_check" (zp_set_tuning): the check INSIDE the one-call provers.  The verdict of the proof's trace stays on the ctx
// (zp_stark_prove_witness_report); anything but SATISFIED ends the call with ZP_ERR_WITNESS and a line naming the first constraint and row, or the
// first non-canonical column and row.  The pieces are csrc/witness_check.hip's, the ones zp_stark_check_witness runs.
int32_t witness_refusal(zp_ctx *ctx) {
    const zp_ctx::WitnessVerdict &v = ctx->last_witness;
    char line[256];
    if (v.rep[0] == ZP_WITNESS_NONCANONICAL)
        snprintf(line, sizeof line, "witness not canonical: %llu trace word(s) >= p, the first in column %llu at row %llu", (unsigned long long)v.rep[5],
                 (unsigned long long)v.rep[6], (unsigned long long)v.rep[7]);
    else
        snprintf(line, sizeof line, "witness violates constraint %llu at row %llu (that constraint at %llu row(s); %llu constraint(s) violated, %llu violations in all)",
                 (unsigned long long)v.rep[2], (unsigned long long)v.rep[1], (unsigned long long)v.counts[v.rep[2]], (unsigned long long)v.rep[4],
                 (unsigned long long)v.rep[3]);
    ctx->err = line;
    return ZP_ERR_WITNESS;
}
// before anything else touches the caller's trace: every word against p.  comm != NULL (the sharded provers): sh.d_trace holds this rank's columns,
// the verdict is the one of the whole trace and every rank reaches it (csrc/witness_sharded.hip)
int32_t prove_check_canonical(zp_ctx *ctx, const Shape &sh, zp_comm *comm = nullptr) {
    zp_ctx::WitnessVerdict &v = ctx->last_witness;
    v.valid = false;
    // the interpreter's requirements (at most 32 slots, canonical constants, checked code) on top of the prover's: a generated kernel needs none of
    // them, but one statement must not be checkable or not by what happens to be registered
    const char *why;
    ZP_ARG(ctx, zpi_program_check(&sh.pg, ZPG_WITNESS, &why), why);
    u64 bad_n, bad_at;
    if (comm) PV_TRY(zpi_witness_sharded_canonical(comm, sh.pg.W, sh.logn, (const u64 *)sh.d_trace, &bad_n, &bad_at));
    else PV_TRY(zpi_witness_canonical(ctx, (const u64 *)sh.d_trace, sh.pg.W * sh.N, &bad_n, &bad_at));
    if (bad_n == 0) return ZP_OK;
    v.counts.assign(sh.pg.K, 0);
    v.first_row.assign(sh.pg.K, ~0ULL);
    zpi_witness_noncanonical_report(sh.pg.K, sh.N, bad_n, bad_at, (uint64_t *)v.rep, nullptr, nullptr);
    memset(v.chal, 0, sizeof v.chal);
    v.valid = true;
    sh.mark("witness refused");
    return witness_refusal(ctx);
}
// as soon as the operands exist: the constraints over (trace, s2, publics | the transcript's stage-2 challenge)
int32_t prove_check_constraints(zp_ctx *ctx, const Shape &sh, const std::vector<u64> &pubs, const u64 *s2, const e3 *chal, zp_comm *comm = nullptr) {
    zp_ctx::WitnessVerdict &v = ctx->last_witness;
    std::vector<u64> pubchal(pubs);
    if (chal) pubchal.insert(pubchal.end(), chal->c, chal->c + 3);
    pubchal.push_back(0);                 // never empty
    v.counts.assign(sh.pg.K, 0);
    v.first_row.assign(sh.pg.K, ~0ULL);
    if (comm)
        PV_TRY(zpi_witness_sharded_constraints(comm, sh.pg, sh.dg, pubchal, (const u64 *)sh.d_trace, s2, sh.logn, (uint64_t *)v.rep, (uint64_t *)v.counts.data(),
                                               (uint64_t *)v.first_row.data()));
    else
        PV_TRY(zpi_witness_constraints(ctx, sh.pg, sh.dg, pubchal, (const u64 *)sh.d_trace, s2, sh.logn, (uint64_t *)v.rep, (uint64_t *)v.counts.data(),
                                       (uint64_t *)v.first_row.data()));
    for (int c = 0; c < 3; c++) v.chal[c] = chal ? chal->c[c] : 0;
    v.valid = true;
    sh.mark("witness checked");
    return v.rep[0] == ZP_WITNESS_SATISFIED ? ZP_OK : witness_refusal(ctx);
}

// zp_stark_prove / zp_stark_prove_bn128: the whole trace on one device
int32_t prove_impl(zp_ctx *ctx, bool bn, const ProveArgs &a) {
    ZpStage stage_(ctx, bn ? "stark_prove_bn128" : "stark_prove");
    ZP_ARG(ctx, a.d_trace, "null pointer");
    Shape sh;
    PV_TRY(make_shape(ctx, bn, a, &sh));
    const size_t W = sh.pg.W, W2 = sh.pg.W2, Wt = sh.Wt, n_s2 = sh.pg.n_s2, Q = sh.pg.Q, N = sh.N, M = sh.M;
    const int logn = sh.logn, logb = sh.logb, logm = sh.logm;
    const u64 shift = sh.shift, wN = sh.wN;
    const uint64_t *d_trace = a.d_trace;
    ZP_ARG(ctx, a.trace_words == (W << logn), "trace_words must be W * 2^logn (W from the program header)");
    DevBufs dev(ctx);
    Transcript tr(ctx, bn);
    const Trees T{ctx, bn};
    PV_TRY(transcript_head(ctx, sh, tr, T, dev));
    std::vector<u64> pubchal(a.h_pubs, a.h_pubs + a.n_pubs);
    const bool check = ctx->tune_prove_check != 0;
    if (check) {          // the trace is resident and untouched: its words, and without stage-2 arguments its constraints, before the first extension
        PV_TRY(prove_check_canonical(ctx, sh));
        if (!n_s2) PV_TRY(prove_check_constraints(ctx, sh, pubchal, nullptr, nullptr));
    }

    // 1. commit the trace (ext has room for the stage-2 columns behind the trace columns).  No coefficient buffer since round 5: the
    //    out-of-domain evaluations come from the resident extension (zp_ood_eval), so the extensions run without their coefficient
    //    store -- on the fused seam kernel where the plan allows it (csrc/ntt.hip) -- and W N 8 bytes per proof are never written
    u64 *ext, *tree1;
    PV_TRY(dev.alloc(Wt * M, &ext));
    const int gt = sh.rows_per_leaf_log(W), g2 = sh.rows_per_leaf_log(W2);
    const size_t Mt = M >> gt, Wtg = W << gt, M2 = M >> g2, W2g = W2 << g2;
    PV_TRY(dev.alloc(T.tree_words(Mt), &tree1));
    PV_TRY(zp_lde(ctx, d_trace, (uint64_t *)ext, nullptr, logn, logb, (int32_t)W, shift));
    PV_TRY(T.commit(ext, Mt, (int)Wtg, tree1));
    u64 root1[4], root2[4] = {0, 0, 0, 0}, rootq[4];
    PV_TRY(T.root(tree1, Mt, root1));
    tr.absorb_root(root1);
    u64 *tree2 = nullptr, *s2_kept = nullptr;
    if (n_s2) {
        const e3 chal = tr.challenge();
        PV_TRY(tr.rc);
        u64 *s2;
        PV_TRY(dev.alloc(W2 * N, &s2));
        PV_TRY(zpi_stage2_columns(ctx, sh.pg, (const u64 *)d_trace, logn, chal.c, s2));
        // the stage-2 columns exist on the trace domain, made with the challenge that binds; nothing has been extended from them yet
        if (check) PV_TRY(prove_check_constraints(ctx, sh, pubchal, s2, &chal));
        PV_TRY(zp_lde(ctx, (const uint64_t *)s2, (uint64_t *)(ext + W * M), nullptr, logn, logb, (int32_t)W2, shift));
        PV_TRY(dev.alloc(T.tree_words(M2), &tree2));
        PV_TRY(T.commit(ext + W * M, M2, (int)W2g, tree2));
        PV_TRY(T.root(tree2, M2, root2));
        s2_kept = s2;                         // the stage-2 columns on the trace domain: read once more for their out-of-domain evaluations
        tr.absorb_root(root2);
        for (int c = 0; c < 3; c++) pubchal.push_back(chal.c[c]);
    }
    const e3 alpha = tr.challenge();
    PV_TRY(tr.rc);

    sh.mark("trace (+stage 2) committed");
    // 2. constraint quotient on the coset
    u64 *fixed, *dq;
    PV_TRY(fixed_columns_cached(ctx, sh, &fixed));
    sh.mark("fixed columns");
    PV_TRY(dev.alloc(3 * M, &dq));
    QuotientOps qo;
    PV_TRY(quotient_operands(ctx, sh, "", alpha, pubchal, dev, &qo));
    if (qo.plug) {       // the generated kernel of this program (zp_stark_set_air_kernel)
        const int hrc = ((zp_air_quotient_fn)qo.plug)((void *)ctx->stream, (const u64 *)ext, (const u64 *)fixed, (u64)M, (u64)1 << logb, qo.d_ops, qo.d_ops + qo.o_ap,
                                                      qo.d_ops + qo.o_zh, (const u64 *)qo.xlo, (const u64 *)qo.xhi, (int)qo.xlb, shift, gl_inv(wN), dq);
        if (hrc != 0) {
            ctx->err = "generated constraint kernel: launch failed (hip error " + std::to_string(hrc) + ")";
            return ZP_ERR_HIP;
        }
        PV_TRY(zp_sync(ctx));
        dev.release(qo.d_ops);
    } else {
        PV_TRY(zp_eval_quotient(ctx, a.h_program, a.program_words, (const uint64_t *)ext, (const uint64_t *)fixed, logm, logb, (const uint64_t *)pubchal.data(),
                                (int32_t)pubchal.size(), (const uint64_t *)qo.apow.data(), (const uint64_t *)qo.zhinv.data(), shift, gl_inv(wN), (uint64_t *)dq));
    }
    sh.mark("quotient evaluated");
    int q_logn = logm;
    size_t Wq = 3;
    u64 *treeq;
    PV_TRY(dev.alloc(T.tree_words(M), &treeq));
    if (Q > 1) {
        u64 *dqcoef, *pad, *pext;
        PV_TRY(split_quotient(ctx, sh, dev, dq, &dqcoef, &pad, &pext));
        PV_TRY(zp_sync(ctx));
        dev.release(pad);
        dev.release(dq);
        dev.release(dqcoef);
        dq = pext;
        q_logn = logn;
        Wq = 3 * Q;
    }
    // BN128 mode: 2^qg rows of the quotient per leaf (rows i, i + M', ...: the matrix reinterpreted as [Wq 2^qg][M'], like a FRI layer),
    // qg the largest with Wq 2^qg <= 48 values = one width-17 permutation per leaf (stark/prover.py: bn128_rows_per_leaf_log)
    const int qg = sh.rows_per_leaf_log(Wq);
    const size_t Mq = M >> qg, Wqg = Wq << qg;
    PV_TRY(T.commit(dq, Mq, (int)Wqg, treeq));
    PV_TRY(T.root(treeq, Mq, rootq));
    tr.absorb_root(rootq);
    const e3 zeta = tr.challenge();
    PV_TRY(tr.rc);

    sh.mark("quotient committed");
    // 3. out-of-domain evaluations FROM VALUES (barycentric form, zp_ood_eval): a polynomial of degree < 2^d is read on a 2^d-point domain it is
    //    known on; the trace and stage-2 columns at zeta and zeta w in ONE pass
    const e3 zeta_w = e3_scale(zeta, wN);
    std::vector<u64> ev_all((Wt + Wq) * 3), ev_next(Wt * 3);
    // (the witness columns are read where they lie CONTIGUOUSLY -- the trace itself and the stage-2 columns, on the trace domain: shift 1, stride 1,
    // 8 N bytes per column; the same numbers as from the 2^logn-point sub-coset of the extension (row stride 2^logb), which costs 16 N)
    PV_TRY(zp_ood_eval(ctx, d_trace, N, 1, (int32_t)W, logn, 1, (const uint64_t *)zeta.c, 1, (uint64_t *)ev_all.data(), (uint64_t *)ev_next.data()));
    if (W2) {
        PV_TRY(zp_ood_eval(ctx, (const uint64_t *)s2_kept, N, 1, (int32_t)W2, logn, 1, (const uint64_t *)zeta.c, 1, (uint64_t *)(ev_all.data() + W * 3),
                           (uint64_t *)(ev_next.data() + W * 3)));
        PV_TRY(zp_sync(ctx));
        dev.release(s2_kept);
    }
    PV_TRY(zp_ood_eval(ctx, (const uint64_t *)dq, M, (size_t)1 << (logm - q_logn), (int32_t)Wq, q_logn, shift, (const uint64_t *)zeta.c, 0,
                       (uint64_t *)(ev_all.data() + Wt * 3), nullptr));
    tr.absorb(ev_all);
    tr.absorb(ev_next);
    const e3 gamma = tr.challenge();
    PV_TRY(tr.rc);

    sh.mark("out-of-domain evaluations");
    // 4. DEEP quotient, 5. FRI
    u64 *df;
    PV_TRY(dev.alloc(3 * M, &df));
    PV_TRY(zp_deep_quotient(ctx, (const uint64_t *)ext, (int32_t)Wt, (const uint64_t *)dq, (int32_t)Wq, logm, (int32_t)Wt, (const uint64_t *)zeta.c, (const uint64_t *)zeta_w.c, (const uint64_t *)gamma.c,
                            (const uint64_t *)ev_all.data(), (const uint64_t *)ev_next.data(), shift, (uint64_t *)df));
    Fri fri;
    PV_TRY(fri_commit(ctx, sh, tr, T, dev, df, &fri));

    // 6. proof of work, then the queries: every tree is whole here
    u64 nonce;
    std::vector<u64> qidx;
    PV_TRY(grind_and_indices(ctx, sh, tr, &nonce, &qidx));
    Opened o_tr, o_s2, o_q;
    std::vector<Opened> fo;
    PV_TRY(open_tree(ctx, T, ext, tree1, Mt, Wtg, qidx, &o_tr));
    if (n_s2) PV_TRY(open_tree(ctx, T, ext + W * M, tree2, M2, W2g, qidx, &o_s2));
    PV_TRY(open_tree(ctx, T, dq, treeq, Mq, Wqg, qidx, &o_q));
    PV_TRY(fri_open(ctx, sh, T, fri, qidx, &fo));
    return write_proof(ctx, sh, tr, {root1, rootq, root2, ev_all, ev_next, fri, nonce, qidx, o_tr, o_q, o_s2, fo});
}

// ======================================================================================================================
// zp_stark_prove_sharded: ONE chunk STARK over the G ranks of a communicator (BASELINE configs[3]) -- what
// eigen_zeth_amd/stark/sharded.py orchestrates in Python, behind one C-ABI call per rank, so that a compiled host (Rust: the side of
// src/prover/provider.rs:358-377) can spread one GenChunkProof over the GPUs of a node.  Every rank passes ITS W/G trace columns and
// ends with the same proof text, byte for byte the text zp_stark_prove writes for the whole trace on one GPU.
//     trace LDE                  columns [W/G][N] -> [W/G][M]                         no exchange
//     trace commitment           rows [W][M/G]: local subtree                          ONE all-to-all, all-gather of G sub-roots
//     stage-2 columns            replicated (a handful of columns)                     broadcast of the witness columns they read
//     constraint quotient        rows, with a blow-up halo (b rows of the next rank)   all-gather of G x Wt x b halo values
//     quotient commitment        rows: local subtree                                   all-gather of the quotient rows, of G sub-roots
//     out-of-domain evaluations  columns (coefficients never move)                     all-gather of the evaluations
//     DEEP quotient              rows                                                  all-gather of the result: "gather before FRI"
//     FRI, proof of work         replicated                                            none
//     query openings             the owner of a row answers                            one all-reduce of values and sub-tree paths

struct ShardTop {                       // the top log2 G levels of a row-sharded tree, known to every rank
    std::vector<std::vector<u64>> levels;   // levels[l]: (G >> l) nodes of 4 words
    u64 root[4];
};

int32_t shard_top(zp_ctx *ctx, const std::vector<u64> &subroots, int G, ShardTop *out) {
    out->levels.clear();
    std::vector<u64> lvl = subroots;
    void *d = nullptr;
    if (G > 1) PV_TRY(zp_dev_alloc(ctx, (size_t)(G / 2) * 12 * 8, &d));
    int32_t rc = ZP_OK;
    for (int n = G; rc == ZP_OK && n > 1; n >>= 1) {
        out->levels.push_back(lvl);
        std::vector<u64> st((size_t)(n / 2) * 12, 0);
        for (int i = 0; i < n / 2; i++) memcpy(&st[12 * (size_t)i], &lvl[8 * (size_t)i], 64);
        rc = zp_h2d(ctx, d, st.data(), st.size() * 8);
        if (rc == ZP_OK) rc = zp_poseidon_perm(ctx, (uint64_t *)d, (size_t)(n / 2));
        if (rc == ZP_OK) rc = zp_d2h(ctx, st.data(), d, st.size() * 8);
        lvl.assign((size_t)(n / 2) * 4, 0);
        for (int i = 0; i < n / 2; i++) memcpy(&lvl[4 * (size_t)i], &st[12 * (size_t)i], 32);
    }
    if (d) (void)zp_dev_free(ctx, d);
    if (rc == ZP_OK) memcpy(out->root, lvl.data(), 32);
    return rc;
}

// local subtree over `rows` u64[Wc][nloc] + all-gather of the sub-roots + the top of the tree
int32_t shard_commit(zp_comm *comm, zp_ctx *ctx, DevBufs &dev, const u64 *rows, size_t nloc, int Wc, int G, u64 **tree_out, ShardTop *top) {
    u64 *tree, *sub;
    PV_TRY(dev.alloc((2 * nloc - 1) * 4, &tree));
    PV_TRY(dev.alloc((size_t)G * 4, &sub));
    PV_TRY(zp_merkle_commit(ctx, (const uint64_t *)rows, nloc, Wc, (uint64_t *)tree));
    PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)(tree + (2 * nloc - 2) * 4), (uint64_t *)sub, 4));
    std::vector<u64> h((size_t)G * 4);
    PV_TRY(zp_d2h(ctx, h.data(), sub, h.size() * 8));
    dev.release(sub);
    PV_TRY(shard_top(ctx, h, G, top));
    *tree_out = tree;
    return ZP_OK;
}

// BN128 mode (16-ary Poseidon-BN254 trees), one row per leaf: the local tree over my nloc = 16^h c rows holds the global tree's nodes of
// levels 0..h under my rows (a group of 16 nodes of level k < h covers 16^(k+1) aligned rows: inside one shard); the c nodes of level h go
// through ONE all-gather and every rank finishes the few levels above them (`top`: a 16-ary tree whose "leaves" are the G c digests)
struct ShardTopBn {
    u64 *ltree = nullptr, *top = nullptr;    // device: local tree (zp_merkle16_nodes(nloc) nodes), top tree (zp_merkle16_nodes(G c) nodes)
    size_t h = 0, ntop = 0;                  // local levels that are global levels; nodes of level h in the whole tree
    u64 root[4];
};
int32_t shard_commit_bn(zp_comm *comm, zp_ctx *ctx, DevBufs &dev, const u64 *rows, size_t nloc, int Wc, int G, ShardTopBn *out) {
    size_t h = 0, c = nloc, off = 0;
    while (c >= 16 && c % 16 == 0) { off += c; c /= 16; h++; }
    out->h = h;
    out->ntop = (size_t)G * c;
    PV_TRY(dev.alloc(zp_merkle16_nodes(nloc) * 4, &out->ltree));
    PV_TRY(dev.alloc(zp_merkle16_nodes(out->ntop) * 4, &out->top));
    PV_TRY(zp_merkle16_commit_bn254(ctx, (const uint64_t *)rows, nloc, Wc, (uint64_t *)out->ltree));
    PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)(out->ltree + off * 4), (uint64_t *)out->top, c * 4));
    PV_TRY(zpi_merkle16_levels_bn254(ctx, out->top, out->ntop));
    return zp_d2h(ctx, out->root, out->top + (zp_merkle16_nodes(out->ntop) - 1) * 4, 32);
}

// [G][C][nloc] (what an all-gather of [C][nloc] row shards delivers) -> [C][G * nloc]
int32_t shard_join(zp_ctx *ctx, const u64 *gathered, u64 *full, int C, size_t nloc, int G) {
    for (int h = 0; h < G; h++)
        ZP_HIP(ctx, hipMemcpy2DAsync(full + (size_t)h * nloc, (size_t)G * nloc * 8, gathered + (size_t)h * C * nloc, nloc * 8, nloc * 8, (size_t)C,
                                     hipMemcpyDeviceToDevice, ctx->stream));
    return ZP_OK;
}

int32_t prove_sharded_impl(zp_comm *comm, zp_ctx *ctx, bool bn, const ProveArgs &a) {
    ZpStage stage_(ctx, bn ? "stark_prove_sharded_bn128" : "stark_prove_sharded");
    const int G = zp_comm_world(comm), rank = zp_comm_rank(comm);
    Shape sh;
    PV_TRY(make_shape(ctx, bn, a, &sh));
    const size_t W = sh.pg.W, W2 = sh.pg.W2, Wt = sh.Wt, n_s2 = sh.pg.n_s2, Q = sh.pg.Q, N = sh.N, M = sh.M, b = (size_t)1 << sh.logb;
    const int logn = sh.logn, logb = sh.logb, logm = sh.logm;
    const u64 shift = sh.shift, wN = sh.wN;
    const uint64_t *d_trace = a.d_trace;
    // what can fail on one rank alone is checked before that rank's first collective
    ZP_ARG(ctx, G >= 1 && M % (size_t)G == 0, "the domain rows must split evenly over the ranks");
    // columns: rank r owns [r wl, min((r + 1) wl, W)), wl = ceil(W / G) -- the last ranks may hold fewer (a 47-column verifier AIR over
    // 8 ranks: 6,6,6,6,6,6,6,5) or none; the exchange moves wl columns per rank, the missing ones as zeros (they land behind column W)
    const size_t wl = (W + (size_t)G - 1) / (size_t)G, nloc = M / G, r0 = (size_t)rank * nloc;
    const size_t wr = (size_t)rank * wl >= W ? 0 : (W - (size_t)rank * wl < wl ? W - (size_t)rank * wl : wl);      // my real columns
    ZP_ARG(ctx, d_trace || wr == 0, "null pointer");
    ZP_ARG(ctx, nloc >= b && nloc % b == 0 && nloc >= 2, "row shards must hold whole blow-up groups");
    ZP_ARG(ctx, a.trace_words == (wr << logn), "trace_words must be (this rank's columns) * 2^logn: ceil(W / world) columns per rank, the tail ranks fewer");
    // BN128 mode (the last STARK before the Groth16 wrap, zp_stark_prove_bn128's text): a leaf of a narrow tree holds 2^g rows i, i + M', ...
    // (Shape::rows_per_leaf_log) -- rows of DIFFERENT shards.  The trace tree is the sharded one and must have one row per leaf
    // (W > 28: the 47-column verifier AIR this mode exists for); the stage-2 and quotient trees are narrow, their columns are whole on
    // every rank anyway (stage 2 is replicated, the quotient is gathered for its out-of-domain evaluation), and 2^g rows per leaf make
    // them M / 2^g permutations against the trace tree's M: they are committed and opened replicated, exactly as prove_impl does
    ZP_ARG(ctx, !bn || sh.rows_per_leaf_log(W) == 0, "BN128 mode shards the trace tree by rows: it needs one row per leaf (more than 28 trace columns)");
    // "prove_check" (set alike on every rank): zp_stark_prove's check over the ranks -- one more exchange, of the RAW trace, and one verdict
    const bool check = ctx->tune_prove_check != 0;
    ZP_ARG(ctx, !check || N / (size_t)G >= 2, "the witness check over the ranks needs at least two trace rows per rank");
    DevBufs dev(ctx);
    Transcript tr(ctx, bn);
    const Trees T{ctx, bn};
    PV_TRY(transcript_head(ctx, sh, tr, T, dev));
    std::vector<u64> pubchal(a.h_pubs, a.h_pubs + a.n_pubs);
    if (check) {          // my columns are resident and untouched: the words, and without stage-2 arguments the constraints, before the first extension
        PV_TRY(prove_check_canonical(ctx, sh, comm));
        if (!n_s2) PV_TRY(prove_check_constraints(ctx, sh, pubchal, nullptr, nullptr, comm));
    }

    // 1. trace: LDE of my columns, ONE exchange columns -> rows, local subtree, sub-roots
    u64 *ext, *tree1 = nullptr;
    ShardTop top1, top2, topq;
    ShardTopBn bt1;
    u64 root1[4], root2[4] = {0, 0, 0, 0}, rootq[4];
    PV_TRY(dev.alloc((Wt > (size_t)G * wl ? Wt : (size_t)G * wl) * nloc, &ext));   // [Wt][nloc]: ALL columns (trace, then stage 2), my rows (room for the exchange's zero columns)
    // (no coefficient buffer since round 5: my columns' out-of-domain evaluations come from d_trace itself, zp_ood_eval on the trace domain)
    {
        u64 *extc, *pack;
        PV_TRY(dev.alloc(wl * M, &extc));
        PV_TRY(dev.alloc(wl * M, &pack));
        if (wr < wl) PV_TRY(zp_dev_zero(ctx, extc + wr * M, (wl - wr) * M * 8));
        if (wr) PV_TRY(zp_lde(ctx, d_trace, (uint64_t *)extc, nullptr, logn, logb, (int32_t)wr, shift));
        PV_TRY(zp_exchange_columns_to_rows(comm, (const uint64_t *)extc, wl, M, (uint64_t *)pack, (uint64_t *)ext));
        PV_TRY(zp_sync(ctx));
        dev.release(extc);
        dev.release(pack);
    }
    if (bn) {
        PV_TRY(shard_commit_bn(comm, ctx, dev, ext, nloc, (int)W, G, &bt1));
        memcpy(root1, bt1.root, 32);
    } else {
        PV_TRY(shard_commit(comm, ctx, dev, ext, nloc, (int)W, G, &tree1, &top1));
        memcpy(root1, top1.root, 32);
    }
    tr.absorb_root(root1);
    const int g2 = sh.rows_per_leaf_log(W2);
    const size_t M2 = M >> g2, W2g = W2 << g2;
    u64 *ext2_kept = nullptr;                     // BN128 mode: the stage-2 extension, whole (its tree's leaves mix rows of all shards)
    u64 *tree2 = nullptr, *s2 = nullptr;          // s2: the stage-2 columns on the trace domain (replicated), kept for their out-of-domain evaluations
    if (n_s2) {
        const e3 chal = tr.challenge();
        PV_TRY(tr.rc);
        u64 *colb, *ext2;
        PV_TRY(dev.alloc(W2 * N, &s2));
        PV_TRY(dev.alloc(3 * N, &colb));           // the (at most three) witness columns an argument reads, on every rank
        PV_TRY(zpi_stage2_columns_sharded(comm, sh.pg, (const u64 *)d_trace, logn, chal.c, colb, s2));
        // the stage-2 columns exist on the trace domain, made with the challenge that binds; nothing has been extended from them yet
        if (check) PV_TRY(prove_check_constraints(ctx, sh, pubchal, s2, &chal, comm));
        PV_TRY(dev.alloc(W2 * M, &ext2));
        PV_TRY(zp_lde(ctx, (const uint64_t *)s2, (uint64_t *)ext2, nullptr, logn, logb, (int32_t)W2, shift));   // replicated: W2 << W
        ZP_HIP(ctx, hipMemcpy2DAsync(ext + W * nloc, nloc * 8, ext2 + r0, M * 8, nloc * 8, W2, hipMemcpyDeviceToDevice, ctx->stream));
        PV_TRY(zp_sync(ctx));
        dev.release(colb);
        if (bn) {
            ext2_kept = ext2;
            PV_TRY(dev.alloc(T.tree_words(M2), &tree2));
            PV_TRY(T.commit(ext2, M2, (int)W2g, tree2));
            PV_TRY(T.root(tree2, M2, root2));
        } else {
            dev.release(ext2);
            PV_TRY(shard_commit(comm, ctx, dev, ext + W * nloc, nloc, (int)W2, G, &tree2, &top2));
            memcpy(root2, top2.root, 32);
        }
        tr.absorb_root(root2);
        for (int c = 0; c < 3; c++) pubchal.push_back(chal.c[c]);
    }
    const e3 alpha = tr.challenge();
    PV_TRY(tr.rc);
    sh.mark("trace exchanged, committed");

    // 2. constraint quotient on my rows (+ the b halo rows of the next rank)
    u64 *dq_l;
    {
        const size_t fwords = zp_fixed_columns_words(a.h_program, a.program_words, logn, logb);
        u64 *fixed, *fx_l;
        PV_TRY(fixed_columns_cached(ctx, sh, &fixed));
        // my window of the two selectors, then the (whole, periodic) extra columns: the layout zp_eval_quotient_rows reads
        PV_TRY(dev.alloc(2 * nloc + (fwords - 2 * M), &fx_l));
        PV_TRY(zp_d2d(ctx, fx_l, fixed + r0, nloc * 8));
        PV_TRY(zp_d2d(ctx, fx_l + nloc, fixed + M + r0, nloc * 8));
        if (fwords > 2 * M) PV_TRY(zp_d2d(ctx, fx_l + 2 * nloc, fixed + 2 * M, (fwords - 2 * M) * 8));
        sh.mark("fixed columns, my window");
        PV_TRY(dev.alloc(3 * nloc, &dq_l));
        // the generated kernel of this program in its row-window form, when the host registered one (zp_stark_set_air_kernel_rows)
        QuotientOps qo;
        PV_TRY(quotient_operands(ctx, sh, "rows:", alpha, pubchal, dev, &qo));
        auto quotient_rows = [&](const u64 *cols, size_t sc, size_t row0, size_t nrows) -> int32_t {
            if (!qo.plug)
                return zp_eval_quotient_rows(ctx, a.h_program, a.program_words, (const uint64_t *)cols, sc, (const uint64_t *)fx_l, nloc, logm, logb, row0, nrows,
                                             (const uint64_t *)pubchal.data(), (int32_t)pubchal.size(), (const uint64_t *)qo.apow.data(),
                                             (const uint64_t *)qo.zhinv.data(), shift, gl_inv(wN), (uint64_t *)dq_l, nloc);
            const int hrc = ((zp_air_quotient_rows_fn)qo.plug)((void *)ctx->stream, cols, (u64)sc, (const u64 *)fx_l, (u64)nloc, (u64)M, (u64)b, (u64)row0, (u64)nrows,
                                                           qo.d_ops, qo.d_ops + qo.o_ap, qo.d_ops + qo.o_zh, (const u64 *)qo.xlo, (const u64 *)qo.xhi, (int)qo.xlb, shift,
                                                           gl_inv(wN), dq_l, (u64)nloc);
            if (hrc != 0) {
                ctx->err = "generated constraint kernel (row window): launch failed (hip error " + std::to_string(hrc) + ")";
                return ZP_ERR_HIP;
            }
            return ZP_OK;
        };
        if (G == 1) {
            PV_TRY(quotient_rows(ext, nloc, 0, M));
        } else {
            u64 *heads, *allh, *buf;
            PV_TRY(dev.alloc(Wt * b, &heads));
            PV_TRY(dev.alloc((size_t)G * Wt * b, &allh));
            PV_TRY(dev.alloc(Wt * (nloc + b), &buf));
            ZP_HIP(ctx, hipMemcpy2DAsync(heads, b * 8, ext, nloc * 8, b * 8, Wt, hipMemcpyDeviceToDevice, ctx->stream));     // my first b rows
            PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)heads, (uint64_t *)allh, Wt * b));
            ZP_HIP(ctx, hipMemcpy2DAsync(buf, (nloc + b) * 8, ext, nloc * 8, nloc * 8, Wt, hipMemcpyDeviceToDevice, ctx->stream));
            ZP_HIP(ctx, hipMemcpy2DAsync(buf + nloc, (nloc + b) * 8, allh + (size_t)((rank + 1) % G) * Wt * b, b * 8, b * 8, Wt, hipMemcpyDeviceToDevice,
                                         ctx->stream));                                                                 // ... of the next rank
            PV_TRY(quotient_rows(buf, nloc + b, r0, nloc));
            PV_TRY(zp_sync(ctx));
            dev.release(heads);
            dev.release(allh);
            dev.release(buf);
        }
        PV_TRY(zp_sync(ctx));
        dev.release(fx_l);
        if (qo.d_ops) dev.release(qo.d_ops);
    }
    sh.mark("quotient on my rows");
    // the quotient is needed whole on every rank: for its out-of-domain evaluation and, with Q > 1, for the coefficients its pieces are slices of
    u64 *dq_whole, *dq_rows = dq_l, *treeq;       // dq_whole: u64[Wq][M], the committed quotient columns (all rows)
    int q_logn = logm;
    size_t Wq = 3;
    {
        u64 *gath;
        PV_TRY(dev.alloc((size_t)G * 3 * nloc, &gath));
        PV_TRY(dev.alloc(3 * M, &dq_whole));
        PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)dq_l, (uint64_t *)gath, 3 * nloc));
        PV_TRY(shard_join(ctx, gath, dq_whole, 3, nloc, G));
        PV_TRY(zp_sync(ctx));
        dev.release(gath);
    }
    if (Q > 1) {
        u64 *dqcoef, *pad, *pext;
        PV_TRY(split_quotient(ctx, sh, dev, dq_whole, &dqcoef, &pad, &pext));
        PV_TRY(dev.alloc(3 * Q * nloc, &dq_rows));
        ZP_HIP(ctx, hipMemcpy2DAsync(dq_rows, nloc * 8, pext + r0, M * 8, nloc * 8, 3 * Q, hipMemcpyDeviceToDevice, ctx->stream));   // my rows of the pieces
        PV_TRY(zp_sync(ctx));
        dev.release(pad);
        dev.release(dq_l);
        dev.release(dqcoef);
        dev.release(dq_whole);
        dq_whole = pext;
        q_logn = logn;
        Wq = 3 * Q;
    }
    const int qg = sh.rows_per_leaf_log(Wq);
    const size_t Mq = M >> qg, Wqg = Wq << qg;
    if (bn) {
        PV_TRY(dev.alloc(T.tree_words(Mq), &treeq));
        PV_TRY(T.commit(dq_whole, Mq, (int)Wqg, treeq));
        PV_TRY(T.root(treeq, Mq, rootq));
    } else {
        PV_TRY(shard_commit(comm, ctx, dev, dq_rows, nloc, (int)Wq, G, &treeq, &topq));
        memcpy(rootq, topq.root, 32);
    }
    tr.absorb_root(rootq);
    const e3 zeta = tr.challenge();
    PV_TRY(tr.rc);
    sh.mark("quotient gathered, committed");

    // 3. out-of-domain evaluations (barycentric form, zp_ood_eval): every rank evaluates ITS trace columns from their values on the trace
    //    domain (d_trace: shift 1, stride 1), the evaluations are all-gathered; the replicated stage-2 columns and quotient on every rank
    const e3 zeta_w = e3_scale(zeta, wN);
    std::vector<u64> ev_all((Wt + Wq) * 3), ev_next(Wt * 3);
    {
        std::vector<u64> mine(2 * wl * 3, 0), all((size_t)G * 2 * wl * 3);
        if (wr) PV_TRY(zp_ood_eval(ctx, d_trace, N, 1, (int32_t)wr, logn, 1, (const uint64_t *)zeta.c, 1, (uint64_t *)mine.data(), (uint64_t *)(mine.data() + wl * 3)));
        u64 *dmine, *dall;
        PV_TRY(dev.alloc(mine.size(), &dmine));
        PV_TRY(dev.alloc(all.size(), &dall));
        PV_TRY(zp_h2d(ctx, dmine, mine.data(), mine.size() * 8));
        PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)dmine, (uint64_t *)dall, mine.size()));
        PV_TRY(zp_d2h(ctx, all.data(), dall, all.size() * 8));
        dev.release(dmine);
        dev.release(dall);
        for (int h = 0; h < G; h++) {
            const size_t c0 = (size_t)h * wl, have = c0 >= W ? 0 : (W - c0 < wl ? W - c0 : wl);
            if (!have) break;
            memcpy(&ev_all[c0 * 3], &all[(size_t)h * 2 * wl * 3], have * 24);
            memcpy(&ev_next[c0 * 3], &all[(size_t)h * 2 * wl * 3 + wl * 3], have * 24);
        }
    }
    if (W2) {
        PV_TRY(zp_ood_eval(ctx, (const uint64_t *)s2, N, 1, (int32_t)W2, logn, 1, (const uint64_t *)zeta.c, 1, (uint64_t *)(ev_all.data() + W * 3),
                           (uint64_t *)(ev_next.data() + W * 3)));
        PV_TRY(zp_sync(ctx));
        dev.release(s2);
    }
    PV_TRY(zp_ood_eval(ctx, (const uint64_t *)dq_whole, M, (size_t)1 << (logm - q_logn), (int32_t)Wq, q_logn, shift, (const uint64_t *)zeta.c, 0,
                       (uint64_t *)(ev_all.data() + Wt * 3), nullptr));
    PV_TRY(zp_sync(ctx));
    if (!bn) dev.release(dq_whole);               // BN128 mode opens its queries from the whole columns
    tr.absorb(ev_all);
    tr.absorb(ev_next);
    const e3 gamma = tr.challenge();
    PV_TRY(tr.rc);
    sh.mark("evaluations gathered");

    // 4. DEEP quotient on my rows, gathered before FRI;  5. FRI (replicated: a layer of the DEEP quotient is 3 columns)
    u64 *df;
    {
        u64 *df_l, *gath;
        PV_TRY(dev.alloc(3 * nloc, &df_l));
        PV_TRY(dev.alloc((size_t)G * 3 * nloc, &gath));
        PV_TRY(dev.alloc(3 * M, &df));
        PV_TRY(zp_deep_quotient_rows(ctx, (const uint64_t *)ext, (int32_t)Wt, nloc, (const uint64_t *)dq_rows, (int32_t)Wq, nloc, logm, r0, nloc, (int32_t)Wt,
                                     (const uint64_t *)zeta.c, (const uint64_t *)zeta_w.c, (const uint64_t *)gamma.c, (const uint64_t *)ev_all.data(),
                                     (const uint64_t *)ev_next.data(), shift, (uint64_t *)df_l, nloc));
        PV_TRY(zp_comm_all_gather(comm, (const uint64_t *)df_l, (uint64_t *)gath, 3 * nloc));
        PV_TRY(shard_join(ctx, gath, df, 3, nloc, G));
        PV_TRY(zp_sync(ctx));
        dev.release(df_l);
        dev.release(gath);
    }
    Fri fri;
    PV_TRY(fri_commit(ctx, sh, tr, T, dev, df, &fri));

    // 6. proof of work, then the queries: the owner of a row answers, one all-reduce spreads the answers
    u64 nonce;
    std::vector<u64> qidx;
    PV_TRY(grind_and_indices(ctx, sh, tr, &nonce, &qidx));
    const size_t nq = qidx.size(), depth = (size_t)logm;
    size_t dl = 0;
    while (((size_t)1 << dl) < nloc) dl++;
    // words of one path of a sharded tree: Goldilocks mode `depth` digests; BN128 mode 16 digests per level of the 16-ary tree
    const size_t pwt = bn ? Trees::levels16(M) * 64 : depth * 4;
    const size_t ltw = bn ? bt1.h * 64 : dl * 4;          // ... of which the owner of the row supplies (the levels inside its sub-tree)
    Opened o_tr, o_s2, o_q;
    o_tr.shape(nq, W, M, pwt);
    if (!bn) {                                            // (Goldilocks mode: one row per leaf in every tree)
        if (n_s2) o_s2.shape(nq, W2, M, pwt);
        o_q.shape(nq, Wq, M, pwt);
    }
    {
        std::vector<int> own;
        std::vector<u64> lidx;
        for (size_t i = 0; i < nq; i++)
            if (qidx[i] >= r0 && qidx[i] < r0 + nloc) { own.push_back((int)i); lidx.push_back(qidx[i] - r0); }
        const size_t no = own.size();
        // layout of the reduced vector: per query [W | W2 | Wq values | local path words of each of the (2 or 3) trees]; BN128 mode: the trace
        // tree alone is sharded: [W values | local path words]
        const size_t ntree = bn ? 1 : n_s2 ? 3 : 2, nval = bn ? W : W + W2 + Wq, per = nval + ntree * ltw;
        const size_t lpw = bn ? Trees::levels16(nloc) * 64 : dl * 4;     // what the local tree's opening returns per query
        std::vector<u64> red(nq * per, 0), tv(no * (W > Wq ? (W > W2 ? W : W2) : (Wq > W2 ? Wq : W2))), tp(no * lpw);
        auto fill = [&](const u64 *mat, size_t Wc, size_t voff, const u64 *tree, size_t poff) -> int32_t {
            if (!no) return ZP_OK;
            PV_TRY(zp_gather_rows(ctx, (const uint64_t *)mat, nloc, (int32_t)Wc, (const uint64_t *)lidx.data(), (int32_t)no, (uint64_t *)tv.data()));
            PV_TRY(T.open(tree, nloc, lidx.data(), (int)no, tp.data()));
            for (size_t k = 0; k < no; k++) {
                memcpy(&red[(size_t)own[k] * per + voff], &tv[k * Wc], Wc * 8);
                memcpy(&red[(size_t)own[k] * per + nval + poff], &tp[k * lpw], ltw * 8);     // the first bt1.h levels / all dl levels
            }
            return ZP_OK;
        };
        PV_TRY(fill(ext, W, 0, bn ? bt1.ltree : tree1, 0));
        if (!bn) {
            if (n_s2) PV_TRY(fill(ext + W * nloc, W2, W, tree2, ltw));
            PV_TRY(fill(dq_rows, Wq, W + W2, treeq, (ntree - 1) * ltw));
        }
        u64 *dred;
        PV_TRY(dev.alloc(red.size(), &dred));
        PV_TRY(zp_h2d(ctx, dred, red.data(), red.size() * 8));
        PV_TRY(zp_comm_all_reduce_sum(comm, (uint64_t *)dred, red.size()));
        PV_TRY(zp_d2h(ctx, red.data(), dred, red.size() * 8));
        dev.release(dred);
        auto paths = [&](std::vector<u64> &dst, size_t poff, const ShardTop &top) {
            for (size_t i = 0; i < nq; i++) {
                memcpy(&dst[i * pwt], &red[i * per + nval + poff], dl * 32);
                u64 node = qidx[i] >> dl;
                for (size_t l = 0; l < top.levels.size(); l++) {         // the top of the path comes from the all-gathered sub-roots
                    memcpy(&dst[i * pwt + (dl + l) * 4], &top.levels[l][(size_t)(node ^ 1) * 4], 32);
                    node >>= 1;
                }
            }
        };
        for (size_t i = 0; i < nq; i++) {
            memcpy(&o_tr.vals[i * W], &red[i * per], W * 8);
            if (bn) continue;
            if (W2) memcpy(&o_s2.vals[i * W2], &red[i * per + W], W2 * 8);
            memcpy(&o_q.vals[i * Wq], &red[i * per + W + W2], Wq * 8);
        }
        if (!bn) {
            paths(o_tr.paths, 0, top1);
            if (n_s2) paths(o_s2.paths, ltw, top2);
            paths(o_q.paths, (ntree - 1) * ltw, topq);
        } else {
            // trace: the levels above the shards from the replicated top tree (its "leaves" are the nodes of level h)
            const size_t tlv = Trees::levels16(bt1.ntop);
            ZP_ARG(ctx, bt1.h + tlv == Trees::levels16(M), "internal: levels of the sharded 16-ary tree do not add up");
            std::vector<u64> tidx(nq), topp(nq * tlv * 64);
            for (size_t i = 0; i < nq; i++) tidx[i] = qidx[i] >> (4 * bt1.h);
            PV_TRY(zp_merkle16_open_batch_bn254(ctx, (const uint64_t *)bt1.top, bt1.ntop, (const uint64_t *)tidx.data(), (int32_t)nq, (uint64_t *)topp.data()));
            for (size_t i = 0; i < nq; i++) {
                memcpy(&o_tr.paths[i * pwt], &red[i * per + nval], ltw * 8);
                memcpy(&o_tr.paths[i * pwt + ltw], &topp[i * tlv * 64], tlv * 64 * 8);
            }
            // stage 2 and quotient: replicated trees over whole columns, opened as prove_impl opens them
            if (n_s2) PV_TRY(open_tree(ctx, T, ext2_kept, tree2, M2, W2g, qidx, &o_s2));
            PV_TRY(open_tree(ctx, T, dq_whole, treeq, Mq, Wqg, qidx, &o_q));
        }
    }
    std::vector<Opened> fo;
    PV_TRY(fri_open(ctx, sh, T, fri, qidx, &fo));

    // every rank writes the text, exactly what zp_stark_prove / zp_stark_prove_bn128 writes, and in BN128 mode keeps the openings record
    return write_proof(ctx, sh, tr, {root1, rootq, root2, ev_all, ev_next, fri, nonce, qidx, o_tr, o_q, o_s2, fo});
}

}  // namespace

int32_t zpi_pool_alloc(zp_ctx *ctx, size_t bytes, void **out) {
    DevBufs b(ctx);
    u64 *p = nullptr;
    const int32_t rc = b.alloc((bytes + 7) / 8, &p);
    if (rc != ZP_OK) return rc;
    b.forget(p);
    *out = p;
    return ZP_OK;
}
void zpi_pool_release(zp_ctx *ctx, void *p, size_t bytes) {
    DevBufs b(ctx);
    b.give_back(p, ((bytes + 7) / 8 ? (bytes + 7) / 8 : 1) * 8);
}
void zpi_sha256(const uint8_t *data, size_t len, uint8_t *out32) { Sha256::digest(data, len, out32); }

extern "C" {

int32_t zp_free_buffer(void *p) {
    free(p);
    return ZP_OK;
}

// A generated constraint kernel (AIR plug-in ABI: stark/air.py writes it, `zpair_<air>_quotient` in its own shared library) for the one-call
// provers of THIS ctx: proofs of the program with this digest evaluate their constraints through it instead of the interpreter -- the same
// values (whole proofs are byte-identical whichever evaluator ran), 0.7 instead of 1.2 ms at 2^21 x 76.  fn = NULL forgets it.  Generated
// kernels read the sparse periodic fixed columns too; the sharded provers take the row-window form registered below.
int32_t zp_stark_set_air_kernel(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, void *quotient_fn) {
    return set_air_kernel(ctx, "", h_program, program_words, quotient_fn);
}
// The ROW-WINDOW form of a generated constraint kernel (`zpair_<air>_quotient_rows` of the same library; round 6): the sharded provers of this ctx
// (zp_stark_prove_sharded, zp_stark_prove_sharded_bn128: every rank evaluates the quotient on ITS rows) use it instead of the interpreter -- same
// values, proofs byte-identical either way.  fn = NULL forgets it.
int32_t zp_stark_set_air_kernel_rows(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, void *quotient_rows_fn) {
    return set_air_kernel(ctx, "rows:", h_program, program_words, quotient_rows_fn);
}

// The WITNESS form of a generated constraint kernel (`zpair_<air>_quotient_witness` of the same library): the constraint check on the trace domain --
// zp_stark_check_witness on this ctx and the one-call provers under "prove_check" -- runs it instead of the interpreter while "witness_kernel" is 1.
// Same reports, word for word.  fn = NULL forgets it.
int32_t zp_stark_set_air_kernel_witness(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, void *witness_fn) {
    return set_air_kernel(ctx, "witness:", h_program, program_words, witness_fn);
}
// ... and its ROW-WINDOW form (`zpair_<air>_quotient_witness_rows`): what a rank of the sharded provers under "prove_check" and of
// zp_stark_check_witness_sharded judges its rows with.  fn = NULL forgets it.
int32_t zp_stark_set_air_kernel_witness_rows(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, void *witness_rows_fn) {
    return set_air_kernel(ctx, "witness_rows:", h_program, program_words, witness_rows_fn);
}

// The verdict of the LAST proof zp_stark_prove / zp_stark_prove_bn128 checked on this ctx ("prove_check" = 1), accepted or refused: zp_stark_check_witness's
// report layout, and the stage-2 challenge it was judged at (the transcript's; zeros without stage-2 arguments or when the trace was not canonical).
int32_t zp_stark_prove_witness_report(zp_ctx *ctx, uint64_t *h_report, uint64_t *h_chal3, uint64_t *h_counts, uint64_t *h_first_row, int32_t n_constraints) {
    if (!ctx) return ZP_ERR_ARG;
    const zp_ctx::WitnessVerdict &v = ctx->last_witness;
    ZP_ARG(ctx, v.valid, "no checked proof has run on this ctx");
    ZP_ARG(ctx, h_report != nullptr, "null pointer");
    ZP_ARG(ctx, n_constraints >= 0 && (size_t)n_constraints == v.counts.size(), "n_constraints is not the program's");
    memcpy(h_report, v.rep, sizeof v.rep);
    if (h_chal3) memcpy(h_chal3, v.chal, sizeof v.chal);
    if (h_counts) memcpy(h_counts, v.counts.data(), v.counts.size() * 8);
    if (h_first_row) memcpy(h_first_row, v.first_row.data(), v.first_row.size() * 8);
    return ZP_OK;
}

// SHA-256 of a constraint program blob: the AIR digest.  out32 = the 32 digest bytes (a proof text names the first 8 as 16 hex digits);
// out_words4 (may be NULL) = the four little-endian 64-bit words, each reduced mod p, that the provers absorb into the transcript.
int32_t zp_program_digest(const uint64_t *h_program, size_t program_words, uint8_t *out32, uint64_t *out_words4) {
    if (!h_program || !out32 || program_words == 0) return ZP_ERR_ARG;
    Sha256::digest((const uint8_t *)h_program, program_words * 8, out32);
    if (out_words4)
        for (int i = 0; i < 4; i++) {
            uint64_t w = 0;
            for (int b = 7; b >= 0; b--) w = (w << 8) | out32[8 * i + b];
            out_words4[i] = w % GL_P;
        }
    return ZP_OK;
}

static int32_t prove_entry(zp_ctx *ctx, bool bn, const ProveArgs &a) {
    if (!ctx) return ZP_ERR_ARG;
    if (a.out_json) *a.out_json = nullptr;
    if (a.out_len) *a.out_len = 0;
    return guarded(ctx, [&] { return prove_impl(ctx, bn, a); });
}

int32_t zp_stark_prove(zp_ctx *ctx, const char *air_name, const uint64_t *h_program, size_t program_words, const uint64_t *d_trace,
                       size_t trace_words, const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, int32_t logb, int32_t fri_logf,
                       int32_t fri_final_log, int32_t n_queries, int32_t pow_bits, char **out_json, size_t *out_len) {
    return prove_entry(ctx, false, {air_name, h_program, program_words, d_trace, trace_words, h_pubs, n_pubs, logn, logb, fri_logf, fri_final_log,
                                    n_queries, pow_bits, out_json, out_len});
}

// the same prover in BN128-hash mode (the last STARK before the Groth16 wrap): 16-ary Poseidon-BN254 trees, transcript over the
// BN254 scalar field, no grinding.  zp_set_poseidon_bn254(ctx, 17, ...) must have installed the tables.
int32_t zp_stark_prove_bn128(zp_ctx *ctx, const char *air_name, const uint64_t *h_program, size_t program_words, const uint64_t *d_trace,
                             size_t trace_words, const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, int32_t logb, int32_t fri_logf,
                             int32_t fri_final_log, int32_t n_queries, char **out_json, size_t *out_len) {
    return prove_entry(ctx, true, {air_name, h_program, program_words, d_trace, trace_words, h_pubs, n_pubs, logn, logb, fri_logf, fri_final_log,
                                   n_queries, 0, out_json, out_len});
}

// Binary openings of the LAST BN128-mode proof made on this ctx (what its text carries under "roots", "fri.roots" and "queries", and the
// transcript behind its challenges), u64 words:
//   [0] "PZOPEN03" [1] n_queries [2] n_trees [3] log2 of the LDE size (bits of a query index), then per tree (trace, quotient, [stage 2], FRI
//   layers): values per leaf, leaves, levels of the 16-ary tree; per tree the root (4 words); per query: the index, then per tree values[width]
//   and path[levels][16][4]; then the transcript: n_blocks, n_rates, the absorbed blocks [n_blocks][16][4], the rate elements the indices
//   were read from [n_rates][16][4], the capacity after every permutation [n_blocks + n_rates - 1][4]; n_challenges and the rate element
//   behind every challenge, in squeeze order [n_challenges][4].
// *out points into the ctx (valid until the next proof on it); ZP_ERR_ARG when there is none.
int32_t zp_stark_openings(zp_ctx *ctx, const uint64_t **out, size_t *words) {
    if (!ctx || !out || !words) return ZP_ERR_ARG;
    ZP_ARG(ctx, !ctx->last_openings.empty(), "no BN128-mode proof has been made on this ctx");
    *out = (const uint64_t *)ctx->last_openings.data();
    *words = ctx->last_openings.size();
    return ZP_OK;
}

int32_t zp_sha256(const uint8_t *data, size_t len, uint8_t *out32) {
    if ((!data && len) || !out32) return ZP_ERR_ARG;
    Sha256::digest(data, len, out32);
    return ZP_OK;
}

// Whatever stops a rank of a sharded proof -- a failed allocation, a HIP error, an exception -- its peers are inside the same call, heading
// for the next collective: zpi_comm_fail takes the communicator down so that they return ZP_ERR_COMM instead of waiting for ever.
static int32_t prove_sharded_entry(zp_comm *comm, bool bn, const ProveArgs &a) {
    if (!comm) return ZP_ERR_ARG;
    zp_ctx *ctx = zpi_comm_ctx(comm);
    if (a.out_json) *a.out_json = nullptr;
    if (a.out_len) *a.out_len = 0;
    const int32_t rc = guarded(ctx, [&] { return prove_sharded_impl(comm, ctx, bn, a); });
    // a refused witness ("prove_check") is a verdict every rank reached from gathered data, at the same point: the communicator lives on
    return rc == ZP_ERR_WITNESS ? rc : zpi_comm_fail(comm, rc);
}

int32_t zp_stark_prove_sharded(zp_comm *comm, const char *air_name, const uint64_t *h_program, size_t program_words, const uint64_t *d_trace_local,
                               size_t trace_words, const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, int32_t logb, int32_t fri_logf,
                               int32_t fri_final_log, int32_t n_queries, int32_t pow_bits, char **out_json, size_t *out_len) {
    return prove_sharded_entry(comm, false, {air_name, h_program, program_words, d_trace_local, trace_words, h_pubs, n_pubs, logn, logb, fri_logf,
                                             fri_final_log, n_queries, pow_bits, out_json, out_len});
}

// the sharded prover in BN128-hash mode: zp_stark_prove_bn128's text (and openings record, on every rank) from W/world columns per rank.
// The trace tree is sharded by rows and must have one row per leaf (more than 28 trace columns: the verifier AIR of the final STARK);
// zp_set_poseidon_bn254(ctx, 17, ...) on every rank's ctx.
int32_t zp_stark_prove_sharded_bn128(zp_comm *comm, const char *air_name, const uint64_t *h_program, size_t program_words, const uint64_t *d_trace_local,
                                     size_t trace_words, const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, int32_t logb, int32_t fri_logf,
                                     int32_t fri_final_log, int32_t n_queries, char **out_json, size_t *out_len) {
    return prove_sharded_entry(comm, true, {air_name, h_program, program_words, d_trace_local, trace_words, h_pubs, n_pubs, logn, logb, fri_logf,
                                            fri_final_log, n_queries, 0, out_json, out_len});
}

}  // extern "C"
