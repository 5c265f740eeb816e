// Internal context shared by the translation units of libzethprover.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zeth_prover.h"
#include "air_program.hpp"
#include "gl.hpp"

#define ZP_ROOT32_DEFAULT 1753635133440165772ULL /* 7^((p-1)/2^32), SURVEY.md 8a-N1 */
#define ZP_SHIFT_DEFAULT 49ULL

struct NttPass {
    int L;         // log2 of the radix; the rounds and the tile width of a launch come from zpi_pass_shape
    int logPprev;  // log2 of the product of the radices of the previous passes
};

struct NttPlan {
    int logn = 0;
    int role = 0;             // zpi_get_plan_role: 0 default, 1 ends / 2 starts in a radix-256 pass (the two sides of the seam kernel)
    bool inverse = false;     // the direction the tables below were made for: what a pass of this plan scales by
    int npass = 0;
    NttPass pass[6];
    int lb = 0;               // twiddle split: w^e = twl[e & (2^lb-1)] * twh[e >> lb]
    u64 *d_twl = nullptr;     // 2^lb entries
    u64 *d_twh = nullptr;     // 2^(logn-lb) entries
    u64 *d_tws = nullptr;     // w_4096^e (direction matched), 4096 entries
    u64 *d_tw1 = nullptr;     // first (transposing) pass: w^(u k) at [u * R + k], all 2^logn of them (null: per-lane chains)
    bool tw1_unavailable = false;   // its allocation failed once: the per-lane chain kernel serves this plan
    u64 *d_itab = nullptr;    // last pass of a plan of >= 3 passes, input side: ninv^inverse * w^(Pp k r) at [k * R + r], Pp and k of the pass before it (null: that pass multiplies its outputs)
    bool itab_unavailable = false;  // its allocation failed once
    u64 w16[8];               // w_16^i (direction matched)
    u64 ninv = 1;
    int j0inv = 0;            // w_16 = (2^12)^j0 ; j0inv = j0^-1 mod 16 (0: not on the power-of-two path)
};

struct CosetTable {  // shift^i * pre, i < 2^logn, two-level
    int logn = 0, lb = 0;
    u64 shift = 0, pre = 0;
    u64 *d_lo = nullptr, *d_hi = nullptr;
};

struct ZpG16Cache;
struct ZpFixedEvalCache;
struct zp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // where every launch of this ctx goes
    hipStream_t own_stream = nullptr;  // created by zp_create (non-blocking); replaced, not destroyed, by zp_set_stream
    std::string err;
    u64 root32 = ZP_ROOT32_DEFAULT;
    u64 coset_shift = ZP_SHIFT_DEFAULT;
    // Poseidon tables (device copies)
    u64 h_rc[360];
    u64 h_mds[144];
    u64 *d_rc = nullptr;
    u32 *d_mds = nullptr;
    bool poseidon_dirty = true;
    bool mds_is_default = false;  // compile-time literal fast path for the documented default matrix
    // plans
    std::map<int, NttPlan> plans;  // key = (logn, inverse, ntt_maxl, ntt_order, role) packed: zpi_get_plan_role
    std::vector<CosetTable> cosets;
    // scratch (six slots, each grown on demand)
    u64 *scratch[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0, 1: NTT ping-pong; 2: LDE coefficients; 3: small uploads; 4: fixed-column periods; 5: zp_ood_eval's weight vector
    size_t scratch_elems[6] = {0, 0, 0, 0, 0, 0};
    // zp_ood_eval: the barycentric weights last made (scratch 5) are for this domain size and point
    bool ood_valid = false;
    int ood_logn = -1;
    u64 ood_y[3] = {0, 0, 0}, ood_root32 = 0;
    // pinned host staging for small transfers (pageable async copies lock/unlock host pages on every call)
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    zp_ctx *msm_helpers[4] = {nullptr, nullptr, nullptr, nullptr};   // zp_groth16_prove: ctxs (streams, MSM arenas) of the MSMs that run beside the first one
    ZpG16Cache *g16_cache = nullptr;   // zp_r1cs_eval_device: the circuit last used, in HBM (csrc/r1cs.hip; freed by zpi_g16_cache_free)
    ZpFixedEvalCache *fixed_eval_cache = nullptr;   // zp_program_fixed_eval_ext_batch: per-entry tables of the programs last used, in HBM (csrc/fixed_eval.hip; freed by zpi_fixed_eval_cache_free)
    int num_cu = 256;
    // experiment knobs (zp_set_tuning): not part of the stable surface
    void *msm_arena = nullptr;    // scratch of zp_msm_bn254*: grows to the largest run, freed by zp_destroy
    size_t msm_arena_bytes = 0;
    int tune_logt12 = 2;          // radix-4096 passes: 2 = tiles of 4 columns (128 KiB, one 1024-thread workgroup per CU), 1 = tiles of 2 columns (64 KiB, two 512-thread workgroups per CU; A/B: profiles/r6_ntt_two_pass_2wg_ab.txt)
    int tune_logt = 4, tune_tpw = 2, tune_logt9 = 4;   // (radix-512 passes: 16-wide tiles of 64 KiB, two workgroups per CU -- 5 to 19 % faster than the 32-wide 128-KiB tile at 2^17 .. 2^27, profiles/r4_logt9_sweep.txt)
    // tiles per workgroup: 2 measured best with the gl_asm.hpp arithmetic (profiles/r2_ntt_sweep.txt)
    int tune_ntt_tw1 = 26;        // largest log size whose first pass multiplies by a full precomputed table (0: always the per-lane chain)
    int tune_ntt_limb = 0;        // 1: register butterflies on the four-limb form of gl_limb.hpp (bit-identical, 17-35 % fewer VALU cycles, but 168 VGPRs and 48 KiB of LDS: 3 workgroups per CU instead of 4 -- measured 4 % slower, profiles/r4_ntt_limb_ab.txt)
    int tune_lde_seam = 1;        // blow-up 2 with radix-256 passes on both sides of the seam: the inverse transform's last pass and the forward one's first in ONE kernel (0: two launches through the coefficient buffer)
    int tune_seam_tpw = 2;        // inverse tiles per workgroup of the seam kernel
    int tune_copy_grid = 0, tune_copy_nt = 1, tune_copy_block = 0, tune_copy_unroll = 0;   // zp_hbm_copy_probe: workgroups (0 = 256: one per CU), policy (1 = non-temporal), lanes per workgroup (0 = 256), 16-byte loads in flight per lane (0 = 4)
    int tune_lde_seam_plans = 1;  // the fused extension may use plans made for it (an inverse plan ending / a forward plan starting in a radix-256 pass) where the default plans do not meet in one (0: default plans only)
    int tune_g16_parallel = 1;    // zp_groth16_prove: the five MSMs of a proof on five streams at once (0: one after the other)
    int tune_ntt_order = 0;       // plan digit order: 0 auto (a radix-512 digit goes last), 1 larger radices first, 2 larger radices last
    int tune_ntt_maxl = 0;        // 0 = 9: largest log2 radix of one NTT pass (10: 1024-thread workgroups, two-pass plans up to 2^20)
    int tune_ntt_small_wave = 0;  // transforms of <= 4096 points: their last six stages inside a wave (DPP / ds_swizzle / ds_bpermute lane exchanges) instead of LDS + a barrier per stage.  0: where it measured faster (<= 64 points), 1: always, 2: never (A/B: profiles/r5_dpp_ab.txt)
    int tune_fri_fold_lanes = 0;  // the FRI fold by 16 with a coset spread over the 16 lanes of a DPP row.  0: where it measured faster (<= 2^16 inputs), 1: always, 2: never (A/B: profiles/r5_dpp_ab.txt)
    int tune_synth_rowwise = 0;   // the synthetic witness's expansion: 1: one 8-byte store per lane and row (round 4), 2: rows staged through LDS and written as column runs, 0: the faster of the two by size (A/B: profiles/r5_synth_fill_ab.txt)
    int tune_p254_block = 0;     // 2: the lane-per-permutation Poseidon-BN254 kernel walks the partial rounds one by one instead of in blocks of four (A/B)
    int tune_p254_scaled = 0;     // 2: the cooperative Poseidon-BN254 kernels walk the unscaled sparse partial rounds (five dependent products per round instead of three; A/B: profiles/r5_p254_scaled_ab.txt)
    int tune_merkle_coop_log = 0; // 0 = 15: tree levels with <= 2^15 nodes go to the 12-lanes-per-node subtree kernel
    int tune_ntt_chunk_log = 0;   // 0 = 28: columns per launch such that a ping-pong scratch buffer is <= 2 GiB
    int tune_p254_bulk_log = 0;   // 0 = 14: Poseidon-BN254 t = 17 launches of >= 2^14 permutations use the lane-per-permutation kernel (31 = never)
    int tune_msm_c = 0;           // 0 = window width chosen from n
    int tune_verify_lane_min = 0;   // 0 = 256: zp_merkle_verify_batch / zp_stark_verify* use the lane-per-opening kernel from this many openings per call on (fewer: the 12-lane walk kernel).  256 (four full waves) is A GUESS until tools/verify_measure.py has run on the device: unmeasured
    int tune_verify16_lane_min = 0; // 0 = 2^14 JOBS (one permutation chain each): zp_merkle16_verify_batch_bn254 / zp_stark_verify*_bn128 hash one job per lane (state in LDS) from this many jobs per call on (fewer: 17 lanes per job).  2^14 is where the lane form wins for commitments: for openings A GUESS until tools/verify_bn128_measure.py has run on the device: unmeasured
    int tune_verify_chain_dev = 1;  // the Fiat-Shamir transcripts (and the commitments of long public-input vectors) of zp_stark_verify* / zp_aggregate_verify* calls with a ctx as ONE sponge-chain launch per call: 0 never, 2 always, 1 (default): where the device beat the parent library at EVERY measured batch size -- today in neither mode (profiles/verify_chains.json: BN128-hash mode wins at 1 and 4 texts, 15.6 -> 10.9 and 61.3 -> 23.9 ms per call, and loses at 16, 25.8 -> 31.4, where the host spreads the header phases over 16 threads and the plan is made on one; Goldilocks mode loses at every size)
    uint64_t verify_counters[4] = {0, 0, 0, 0};   // zp_verify_counters: chain launches, chain steps run on the device, public-input commitments made on the device, texts that took the host sponge on the device path
    int tune_msm_chunk_log = 0;   // 0 = default (2^24 points per Pippenger run)
    int tune_fixed_eval_dev_min = 1 << 15;   // zp_program_fixed_eval_ext_batch with a ctx: calls of fewer (points x sparse entries) run on the host (0: always the device; < 0 restores this default).  2^15: from ~12.5 ns per entry on 16 host threads against ~0.5 ms per device call (profiles/r12_fixed_eval_batch.json: every size measured there is above it and the device wins, 10x at one point of 4.4 x 10^5 entries); not measured AT the crossover
    int tune_witness_kernel = 1;  // the constraint check (zp_stark_check_witness on a ctx, the provers under "prove_check") runs the program's GENERATED witness kernel when one is registered (zp_stark_set_air_kernel_witness); 0: always the interpreter.  Same reports either way (figures: profiles/witness_check_inproof.json)
    int tune_prove_check = 0;     // 1: zp_stark_prove / zp_stark_prove_bn128 check the trace inside the proof (canonical words first, the constraints at the transcript's own stage-2 challenge) and refuse a false witness with ZP_ERR_WITNESS; 0: they prove whatever they are handed
    int tune_s2_diag_merge = 1;   // zp_stark_diagnose_stage2 on a ctx: a wave whose live lanes all carry ONE key issues its table atomics from one lane (the wave_count idea of csrc/msm.hip); 0: every lane its own.  Same records either way (A/B: tools/stage2_diag_measure.py)
    // zp_stark_prove: device buffers kept between proofs (chunk after chunk has the same shapes; hipMalloc / hipFree of ~20 buffers
    // cost milliseconds per proof) and the LDE of the two boundary selectors per (logn, logb, shift, root)
    std::multimap<size_t, void *> prove_pool;
    size_t prove_pool_bytes = 0;
    std::map<std::string, u64 *> prove_fixed;
    size_t prove_fixed_bytes = 0;
    std::map<std::string, void *> air_kernels;   // 64-hex-digit program digest -> generated constraint kernel (AIR plug-in ABI): zp_stark_set_air_kernel
    struct DigestEntry { std::vector<uint64_t> words; uint8_t dg[32]; };
    std::vector<DigestEntry> digest_cache;   // SHA-256 of the large constraint programs seen last (csrc/prove.hip: program_digest)
    struct WitnessVerdict { bool valid = false; u64 rep[8], chal[3]; std::vector<u64> counts, first_row; } last_witness;   // the last proof checked under "prove_check" (zp_stark_prove_witness_report)
    std::vector<u64> last_openings;          // BN128-hash mode: roots, query indices, opened values and paths of the last proof, binary (zp_stark_openings)
    // per-launch event profiling (zp_set_profiling)
    bool profiling = false;
    struct PassEv { hipEvent_t a, b; int radix_log; };
    std::vector<PassEv> pass_events;
    struct StageEv { hipEvent_t a, b; const char *name; };
    std::vector<StageEv> stage_events;
};

// brackets one C-ABI compute call with HIP events on the ctx stream when profiling is on (zp_stage_timings)
struct ZpStage {
    zp_ctx *ctx;
    zp_ctx::StageEv ev;
    bool on;
    ZpStage(zp_ctx *c, const char *name) : ctx(c), on(c && c->profiling) {
        if (c) (void)hipSetDevice(c->device);   // a host thread may alternate between ctxs of different GPUs
        if (on) {
            ev.name = name;
            on = hipEventCreate(&ev.a) == hipSuccess && hipEventCreate(&ev.b) == hipSuccess &&
                 hipEventRecord(ev.a, ctx->stream) == hipSuccess;
        }
    }
    ~ZpStage() {
        if (on && hipEventRecord(ev.b, ctx->stream) == hipSuccess) ctx->stage_events.push_back(ev);
    }
};

// first statement of every entry point that touches the device without a ZpStage
#define ZP_BIND(ctx) do { if (ctx) (void)hipSetDevice((ctx)->device); } while (0)

#define ZP_HIP(ctx, call)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return e_ == hipErrorOutOfMemory ? ZP_ERR_NOMEM : ZP_ERR_HIP;                    \
        }                                                                                    \
    } while (0)

#define ZP_ARG(ctx, cond, msg)                                                               \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            (ctx)->err = std::string("bad argument: ") + (msg);                              \
            return ZP_ERR_ARG;                                                               \
        }                                                                                    \
    } while (0)

#define ZP_TRY(expr)                                                                         \
    do {                                                                                     \
        int32_t rc_ = (expr);                                                                \
        if (rc_ != ZP_OK) return rc_;                                                        \
    } while (0)

// host work over items 0 .. n - 1 on T threads: work(first, end) on the t-th of T near-equal ranges, empty ranges skipped; returns once all have ended
template <class Work>
void zpi_split_over_threads(size_t n, int T, Work work) {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++) {
        const size_t a = n * t / T, b = n * (t + 1) / T;
        if (a < b) pool.emplace_back(work, a, b);
    }
    for (auto &th : pool) th.join();
}

// how many host threads an entry point with a `threads` argument uses: threads <= 0 is one per core; at most 16
inline unsigned zpi_host_threads(int threads) {
    const unsigned nt = threads > 0 ? (unsigned)threads : std::thread::hardware_concurrency();
    return nt < 1 ? 1 : nt > 16 ? 16 : nt;
}
// work(t) for every t < T: T - 1 threads are started, share 0 runs here, and so does the share of every thread that could not be started; returns
// once all have ended
template <class Work>
void zpi_over_threads(unsigned T, Work work) {
    std::vector<std::thread> pool;
    unsigned started = 0;
    try { for (unsigned t = 1; t < T; t++) { pool.emplace_back(work, t); started = t; } } catch (...) {}
    work(0u);
    for (unsigned t = started + 1; t < T; t++) work(t);
    for (auto &th : pool) th.join();
}

// internal helpers implemented across the .hip files
int32_t zpi_scratch(zp_ctx *ctx, int which, size_t elems, u64 **out);
int32_t zpi_pinned(zp_ctx *ctx, size_t bytes, void **out);
// small copies through the pinned staging buffer (synchronous on the ctx stream)
int32_t zpi_d2h_small(zp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int32_t zpi_h2d_small(zp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
// a copy of any size, done when the call returns: through the pinned buffer when small, else an async copy and a synchronisation of the ctx stream
int32_t zpi_d2h(zp_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int32_t zpi_h2d(zp_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int32_t zpi_upload(zp_ctx *ctx, const std::vector<u64> &h, u64 **d);   // a new device buffer holding h (synchronous)
#define ZP_SMALL_COPY (4u << 20)
// csrc/stark.hip: nq query indices up, the gather kernel that launch(d_idx, d_out) enqueues, `total` words down to h_out; staging: a small round trip
// may go through the page-locked staging buffer, which the kernel then reads and writes directly
int32_t zpi_query_round_trip(zp_ctx *ctx, const u64 *h_idx, int nq, u64 total, u64 *h_out, bool staging, const std::function<void(const u64 *, u64 *)> &launch);
int32_t zpi_get_plan(zp_ctx *ctx, int logn, bool inverse, NttPlan **out);
int32_t zpi_get_plan_role(zp_ctx *ctx, int logn, bool inverse, int role, NttPlan **out);   // role 1 / 2: ends / starts with a radix-256 pass (csrc/ntt.hip)
// The shape of one pass of radix 2^L: register rounds of radix 2^A1, 2^A2, 2^A3 on tiles of 2^logT columns.  Decided by the knobs ntt_logt / ntt_logt9 / ntt_logt12, by whether the transform has more than
// 2^28 rows (big) and, for L = 12, by whether the pass transposes (a first pass) or multiplies (inter-pass twiddle, 1/N or a coset power).  A1 == 0: no kernel is built for this pass.
struct NttPassShape { int A1, A2, A3, logT; };
NttPassShape zpi_pass_shape(const zp_ctx *ctx, int L, bool big, bool transpose, bool multiplies);
NttPassShape zpi_plan_pass_shape(const zp_ctx *ctx, const NttPlan *pl, int i);   // pass i of a plan run on its own (no post-scale)
bool zpi_plan_uses_itab(const NttPlan *pl);                                         // the last pass multiplies its input rows by the plan's table (d_itab), the pass before it runs plain
bool zpi_plan_uses_tw1(const zp_ctx *ctx, const NttPlan *pl);                      // the first pass multiplies by the plan's full table (d_tw1)
int32_t zpi_lde_plan_json(zp_ctx *ctx, int logn, int want_coef, std::string *out);           // which path zp_lde takes at this size
int32_t zpi_get_coset(zp_ctx *ctx, int logn, u64 shift, u64 pre, CosetTable **out);
int32_t zpi_poseidon_sync_tables(zp_ctx *ctx);
int32_t zpi_poseidon_chains(zp_ctx *ctx, const u64 *d_blocks, const unsigned char *d_absorb, const unsigned int *d_first, int nchains, u64 *d_out);
// the width-17 twin (csrc/poseidon_bn254.hip: sponge_chains254_kernel, three chains to a workgroup): d_blocks u64[nsteps][16][4] standard form < r, d_out u64[nsteps][16][4]
// the rate after every step
int32_t zpi_poseidon254_chains(zp_ctx *ctx, const u64 *d_blocks, const unsigned char *d_absorb, const unsigned int *d_first, int nchains, u64 *d_out);
// either mode's chains from host buffers (the verifier's transcripts; zp_poseidon_bn254_chains): one upload, one launch, one download, one synchronisation.
// h_blocks / h_rates: 8 words per step (Goldilocks), 64 (BN254); h_first[nchains] steps in all, > 0.  Counted in ctx->verify_counters
int32_t zpi_poseidon_chains_host(zp_ctx *ctx, const u64 *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int nchains, u64 *h_rates);
int32_t zpi_poseidon254_chains_host(zp_ctx *ctx, const u64 *h_blocks, const uint8_t *h_absorb, const uint32_t *h_first, int nchains, u64 *h_rates);
// the commitments long public-input vectors enter a transcript as, of every such text of a call: canonical values in, h_out4 u64[n][4]; the trees are
// built by the prover's kernels (rows of 8, binary: zp_merkle_commit_rows's; rows of 48, 16-ary: zp_merkle16_commit_bn254's); one synchronisation
int32_t zpi_publics_digests(zp_ctx *ctx, const std::vector<const std::vector<u64> *> &pubs, u64 *h_out4);
int32_t zpi_publics_digests_bn254(zp_ctx *ctx, const std::vector<const std::vector<u64> *> &pubs, u64 *h_out4);
int32_t zpi_poseidon_openings_walk(zp_ctx *ctx, const u64 *d_op, const u64 *d_vals, u64 mw, const u64 *d_index, const u64 *d_sib, const u64 *d_sib_off,
                                   size_t count, u64 *d_inputs, u64 *d_digests);
// one Merkle opening a verifier checks: `width` leaf values, `depth` siblings of four words (bottom-up), the leaf's position, and which of the
// caller's roots it must hash to.  Host pointers; the words are canonical (the caller reduces what it read from a text)
// A 16-ary Poseidon-BN254 opening (csrc/poseidon_bn254.hip) uses the same record: `path` is [depth][16][4] raw words (the whole group of every level),
// `depth` the number of levels above `leaves` leaves (which need not be a power of 16), the root one element of four words
struct ZpOpening { const u64 *values, *path; u64 index; uint32_t width, depth, root_slot; u64 leaves; };
// ok[o] = 1 iff opening o hashes to roots[4 * root_slot ..): every opening of a call in ONE launch (csrc/poseidon.hip).  Openings of one
// (width, depth) should be adjacent: a wave then walks one tree shape
int32_t zpi_merkle_verify_openings(zp_ctx *ctx, const ZpOpening *ops, size_t n, const u64 *h_roots, size_t n_roots, uint8_t *ok);
// the same for 16-ary Poseidon-BN254 openings: every hash of every opening is one JOB (a leaf chain, or one level's group), all jobs of a call in ONE
// launch; ok[o] = the AND of opening o's jobs.  Widths, level counts and indices are validated here, before the launch
int32_t zpi_merkle16_verify_openings_bn254(zp_ctx *ctx, const ZpOpening *ops, size_t n, const u64 *h_roots, size_t n_roots, uint8_t *ok);
// the t = 17 tables installed on the ctx's device as the host verifier takes them: Montgomery limbs, rc [(8 + rp) * 17][9], mds [17 * 17][9]
int32_t zpi_p254_host_tables(zp_ctx *ctx, std::vector<u32> *rc, std::vector<u32> *mds, int *rp);
// run the transform on W columns; in/out column strides are 2^logn (or in_valid for zero-padded input)
struct NttRunOpts {
    const CosetTable *post_scale = nullptr;  // multiply output i by table(i) (last pass)
    int in_valid_log = -1;                   // >=0: input columns have 2^in_valid_log elements, rest is zero
    bool seam_last = false;                  // the passes before the last only: the last one runs inside lde_seam_kernel
};
// zp_fixed_columns; only_pub: refresh just the columns that hold public inputs inside a buffer whose other columns are already built
int32_t zpi_fixed_columns_build(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *h_pub, int32_t n_pub, int32_t logn, int32_t logb,
                                uint64_t shift, uint64_t *d_out, size_t out_words, bool only_pub);
// its first half: one period of every (selected) sparse column in scratch 4, behind two selector columns of sel_rows rows each (0: none) unless only_pub
int32_t zpi_fixed_periods_build(zp_ctx *ctx, const uint64_t *h_program, const std::vector<ZpFixedCol> &fxc, const uint64_t *h_pub, size_t sel_rows, bool only_pub,
                                u64 **d_in, size_t *in_words);
// The device copy of a parsed program that both row interpreters read (csrc/stark.hip), in scratch 3: header, constants and instructions -- NOT the
// sparse columns' entry tables behind them, which no kernel reads (for a verifier AIR they are 7 MB of the blob: this upload was 16 ms of a 63 ms
// aggregation STARK) | publics and challenges, one zero word behind them | the caller's extra vectors, one after the other | (offset, index mask) of
// every sparse column's period of 2^(lp + logb) words.  One upload, done when the call returns.
struct ZpSpan { const u64 *p; size_t n; };
struct ZpProgramDev { const u64 *consts, *ins, *pubchal, *extra, *fx_tab; };
int32_t zpi_program_upload(zp_ctx *ctx, const ZpProgram &pg, ZpSpan pubchal, std::initializer_list<ZpSpan> extra, int logb, ZpProgramDev *out);
// zp_stark_check_witness on a ctx (csrc/witness_check.hip): arguments validated by the caller (csrc/witness_host.hip), pubchal = publics then the challenge
int32_t zpi_witness_check_device(zp_ctx *ctx, const ZpProgram &pg, const std::vector<u64> &pubchal, const u64 *d_trace, int logn, uint64_t *h_report,
                                 uint64_t *h_counts, uint64_t *h_first_row);
// its three pieces (csrc/witness_check.hip), shared with the one-call provers under "prove_check" (csrc/prove.hip): the canonical pass; the report of a
// non-canonical trace; the constraints over (trace, GIVEN stage-2 columns, publics then challenge) -- through the program's generated witness kernel when
// dg32 names one and "witness_kernel" allows it, else the interpreter
int32_t zpi_witness_canonical(zp_ctx *ctx, const u64 *d_trace, size_t total, u64 *bad_n, u64 *bad_at);
void zpi_witness_noncanonical_report(size_t K, size_t N, u64 bad_n, u64 bad_at, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row);
int32_t zpi_witness_constraints(zp_ctx *ctx, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace, const u64 *d_s2,
                                int logn, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row);
// the launch behind it, the result [first key][first_row: K][counts: K] left on the device in d_res.  win != NULL: rows [row0, row0 + nrows) only, d_trace
// u64[W][stride] with one halo row at index nrows unless nrows == N; d_s2 whole (`<symbol>_witness_rows` or witness_program_kernel<true>)
struct ZpWitnessWindow { size_t stride, row0, nrows; };
int32_t zpi_witness_launch(zp_ctx *ctx, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace, const u64 *d_s2, int logn,
                           const ZpWitnessWindow *win, u64 *d_res);
// zp_stark_diagnose_stage2 on a ctx (csrc/stage2_diag.hip): arguments validated by the caller (csrc/stage2_diag_host.hip), which also owns the records of
// a trace with words >= p; h_diag u64[n_s2][ZP_S2_WORDS] is written only when ZP_OK is returned
int32_t zpi_stage2_diag_device(zp_ctx *ctx, const ZpProgram &pg, const u64 *d_trace, int logn, uint64_t *h_diag);
void zpi_stage2_diag_noncanonical(const ZpProgram &pg, uint64_t *h_diag);
// csrc/prove.hip: the SHA-256 of a program through the ctx's cache of large blobs; the key a generated kernel of that digest is kept under
void zpi_program_digest_cached(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, uint8_t dg[32]);
std::string zpi_air_kernel_key(const char *form, const uint8_t dg[32]);
// device buffers from / back to the per-ctx pool of zp_stark_prove (csrc/prove.hip): everything runs on the ctx stream, so reuse is ordered
int32_t zpi_pool_alloc(zp_ctx *ctx, size_t bytes, void **out);
void zpi_pool_release(zp_ctx *ctx, void *p, size_t bytes);
void zpi_sha256(const uint8_t *data, size_t len, uint8_t *out32);
void zpi_g16_cache_free(zp_ctx *ctx);
void zpi_fixed_eval_cache_free(zp_ctx *ctx);
// the sparse fixed columns of a validated program at n_points points in two launches (csrc/fixed_eval.hip): h_sparse u64[n_points][cols.size()][3];
// h_on_domain[i] = 1 (and zero rows) where a denominator of point i vanished.  Inputs canonical, every lp <= logn: csrc/verify.hip checks before it calls
int32_t zpi_fixed_eval_device(zp_ctx *ctx, const uint64_t *h_program, size_t program_words, const std::vector<ZpFixedCol> &cols, const uint64_t *h_pubchal,
                              int32_t n_pubchal, int32_t logn, uint64_t root32, const uint64_t *h_zeta, int32_t n_points, uint64_t *h_sparse, uint8_t *h_on_domain);
int32_t zpi_r1cs_poseidon17(zp_ctx *ctx, const u64 *d_inst, size_t i0, size_t count, u64 *d_w, unsigned char *d_set, u64 *d_a, u64 *d_b, u64 *d_c,
                            unsigned long long *d_flags, int *rp_out);
int32_t zpi_merkle16_levels_bn254(zp_ctx *ctx, u64 *d_tree, size_t n);   // the levels above n digests at the head of a 16-ary tree buffer (csrc/poseidon_bn254.hip)
struct zp_comm;
zp_ctx *zpi_comm_ctx(const zp_comm *comm);      // the ctx a communicator was created on (csrc/comm.hip)
int32_t zpi_comm_fail(zp_comm *comm, int32_t rc);   // rc != ZP_OK: kill the communicator (no peer waits for this rank); returns rc
// the witness check over the ranks (csrc/witness_sharded.hip): every rank passes its columns and receives the same answer.  Collectives inside: a
// caller hands a failure to zpi_comm_fail.  canonical: words >= p over all ranks and the GLOBAL index c N + r of the first; constraints: given the
// stage-2 columns whole (or NULL), the report of zpi_witness_constraints for the whole trace; the stage-2 columns themselves, as the sharded prover makes them
int32_t zpi_witness_sharded_canonical(zp_comm *comm, size_t W, int logn, const u64 *d_trace_local, u64 *bad_n, u64 *bad_at);
int32_t zpi_witness_sharded_constraints(zp_comm *comm, const ZpProgram &pg, const uint8_t *dg32, const std::vector<u64> &pubchal, const u64 *d_trace_local,
                                        const u64 *d_s2, int logn, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row);
// csrc/stage2.hip: the k-th stage-2 argument of pg (st = pg.stage2 + 4 k) from three whole columns on this device (c unused by a grand product); writes its
// planes at d_s2 + *at * N, advances *at
int32_t zpi_stage2_argument(zp_ctx *ctx, const u64 *st, const u64 *a, const u64 *b, const u64 *c, size_t N, const u64 g[3], u64 *d_s2, size_t *at);
// all of them, columns taken from a whole trace u64[W][N] on this device
int32_t zpi_stage2_columns(zp_ctx *ctx, const ZpProgram &pg, const u64 *d_trace, int logn, const u64 g[3], u64 *d_s2);
int32_t zpi_stage2_columns_sharded(zp_comm *comm, const ZpProgram &pg, const u64 *d_trace_local, int logn, const u64 g[3], u64 *d_colb, u64 *d_s2);
// csrc/witness_host.hip: the argument checks of zp_stark_check_witness and its sharded twin, the parsed program and [publics | challenge | 0]; NULL or the refusal
const char *zpi_witness_args(const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words, int world, int rank,
                             const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, const uint64_t *h_chal3, const uint64_t *h_report, const uint64_t *h_counts,
                             const uint64_t *h_first_row, int32_t n_constraints, ZpProgram *pg, std::vector<u64> *pubchal);
// the slice rule of the sharded entry points: with k = ceil(n / world), rank r owns [r k, min((r + 1) k, n)) -- the tail ranks fewer, or none
inline void zpi_shard_range(size_t n, int world, int rank, size_t *first, size_t *count) {
    const size_t k = (n + (size_t)world - 1) / (size_t)world, lo = (size_t)rank * k;
    *first = lo < n ? lo : n;
    *count = lo >= n ? 0 : (n - lo < k ? n - lo : k);
}
// out = the sum, in order, of `count` affine BN254 points in the zp_msm_bn254 layout (g2 = 0: u32[16] each; 1: G2, u32[32]; all-zero = infinity),
// on the host: the partial sums of a sharded MSM (csrc/msm.hip)
void zpi_bn254_affine_sum(int g2, const uint32_t *pts, int count, uint32_t *out);
int32_t zpi_twiddle_rows(zp_ctx *ctx, u64 *d_rows, int logn_row, int W, u64 row0, int logn_total, bool inverse);
int32_t zpi_lde(zp_ctx *ctx, const u64 *d_in, u64 *d_out, u64 *d_coef, int logn, int logb, int W, u64 shift);
int32_t zpi_ntt_run(zp_ctx *ctx, const u64 *d_in, u64 *d_out, int logn, int W, bool inverse,
                    const NttRunOpts &opts);
