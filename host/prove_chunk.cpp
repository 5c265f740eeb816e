// A compiled host above the C-ABI -- what a Rust prover service (the reference's side of the boundary is compiled code:
// src/prover/provider.rs talks to such a service) does for one GenChunkProof, written in C++ because this image has no Rust
// toolchain: load libzethprover.so's entry points, put the witness in HBM, call zp_stark_prove, hand the proof text on.
// Nothing but include/zeth_prover.h is used -- no Python, no torch, no compiler at run time (the AIR is a data blob).
//
// usage: prove_chunk <program.bin> <trace.bin> <publics.bin> <logn> <logb> <fri_logf> <fri_final_log> <n_queries> <pow_bits> <out.json> [air_name
//                     [rank world id-file [run-nonce]]]
//   with rank / world / id-file: ONE proof over `world` GPUs, one process per GPU (zp_stark_prove_sharded on an RCCL communicator; rank 0
//   publishes the 128-byte RCCL id in <id-file>, the others wait for the record that carries this run's nonce: host/rendezvous.hpp).  Rank r reads only ITS columns of trace.bin (ceil(W / world) per rank, the tail ranks fewer) and drives GPU r;
//   every rank obtains the same proof text (rank 0 writes <out.json>), byte for byte the single-GPU text.
//   --check (anywhere on the line): before proving, zp_stark_check_witness judges the trace against the program on the GPU, in HBM -- in a sharded
//   run zp_stark_check_witness_sharded, every rank on ITS columns, all with the same report -- and prints the report (rank 0) as ONE JSON line
//   {"witness_check":{"verdict":..,"first_row":..,"first_constraint":..,"violations":..,"violated_constraints":..,"noncanonical":..,
//   "first_noncanonical":[column,row]}} (null where the report says none); a trace that is not satisfied ends the run with exit status 3, unproven.
//   --check-prove: the check runs INSIDE the proof instead (zp_set_tuning "prove_check": canonical words, then the constraints at the proof's own
//   stage-2 challenge; a sharded run checks over its ranks); the same JSON line (zp_stark_prove_witness_report; rank 0 prints it) in front of the
//   result, and a refusal (ZP_ERR_WITNESS, on every rank) ends the run with exit status 3, unproven.
//   --diagnose (one GPU; with --check or --check-prove): after a refusal, zp_stark_diagnose_stage2 compares the columns of the program's permutations
//   and lookups as multisets, in HBM, and one line per argument that fails says which cell is wrong -- the report above names only row N - 1, where
//   the running product or sum fails to close:  {"stage2":{"argument":j,"kind":"lookup","column":"a","row":..,"value":..,"lhs":..,"rhs":..}}
//   (the smallest row of column a holding an unbalanced value, lhs = its occurrences in a, rhs = its count on the other side; when only the other
//   column holds one, that column -- "b" or "t" -- and its smallest such row).
//   program.bin : the constraint program blob (u64 words, layout in the header)
//   trace.bin   : u64[W][2^logn] column-major, canonical values
//   publics.bin : u64[n_pub]
// build: make -C host   (g++ -I../include prove_chunk.cpp -L../eigen_zeth_amd/csrc -lzethprover)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/zeth_prover.h"
#include "rendezvous.hpp"

static std::vector<uint64_t> read_words(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> v((size_t)n / 8);
    if (n % 8 || fread(v.data(), 8, v.size(), f) != v.size()) { fprintf(stderr, "bad file %s\n", path); exit(2); }
    fclose(f);
    return v;
}

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        const int32_t rc_ = (call);                                                                   \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, ctx ? zp_last_error(ctx) : "no context"); return 1; } \
    } while (0)

// the report of zp_stark_check_witness as one JSON line; true: satisfied
static bool print_report(const uint64_t *r) {
    auto opt = [](uint64_t v) { return v == ~0ULL ? std::string("null") : std::to_string((unsigned long long)v); };
    static const char *names[3] = {"satisfied", "violated", "noncanonical"};
    printf("{\"witness_check\":{\"verdict\":\"%s\",\"first_row\":%s,\"first_constraint\":%s,\"violations\":%llu,\"violated_constraints\":%llu,"
           "\"noncanonical\":%llu,\"first_noncanonical\":%s}}\n",
           r[0] < 3 ? names[r[0]] : "?", opt(r[1]).c_str(), opt(r[2]).c_str(), (unsigned long long)r[3], (unsigned long long)r[4], (unsigned long long)r[5],
           r[6] == ~0ULL ? "null" : ("[" + opt(r[6]) + "," + opt(r[7]) + "]").c_str());
    fflush(stdout);
    return r[0] == ZP_WITNESS_SATISFIED;
}

// zp_stark_diagnose_stage2 on the refused trace: one JSON line per argument that fails
static int32_t print_diagnosis(zp_ctx *ctx, const std::vector<uint64_t> &program, const void *d_trace, size_t trace_words, int logn) {
    const size_t n = (size_t)program[10];              // n_stage2 of the header; the library checks it against the blob
    if (n == 0 || n > 65536) return 0;
    std::vector<uint64_t> diag(n * ZP_S2_WORDS);
    const int32_t rc = zp_stark_diagnose_stage2(ctx, program.data(), program.size(), (const uint64_t *)d_trace, trace_words, logn, diag.data(), (int32_t)n, 0);
    if (rc != 0) return rc;
    for (size_t j = 0; j < n; j++) {
        const uint64_t *r = diag.data() + j * ZP_S2_WORDS;
        if (r[0] != ZP_S2_FAILS) continue;
        const uint64_t *s = r[3] != ~0ULL ? r + 3 : r + 7;         // (row, value, lhs, rhs) of column a, else of the other column
        printf("{\"stage2\":{\"argument\":%zu,\"kind\":\"%s\",\"column\":\"%s\",\"row\":%llu,\"value\":%llu,\"lhs\":%llu,\"rhs\":%llu}}\n", j,
               r[1] == 1 ? "permutation" : "lookup", s == r + 3 ? "a" : r[1] == 1 ? "b" : "t", (unsigned long long)s[0], (unsigned long long)s[1],
               (unsigned long long)s[2], (unsigned long long)s[3]);
    }
    fflush(stdout);
    return 0;
}

int main(int argc, char **argv) {
    bool check = false, check_prove = false, diagnose = false;
    {
        int n = 1;
        for (int i = 1; i < argc; i++) {
            if (strcmp(argv[i], "--check") == 0) check = true;
            else if (strcmp(argv[i], "--check-prove") == 0) check_prove = true;
            else if (strcmp(argv[i], "--diagnose") == 0) diagnose = true;
            else argv[n++] = argv[i];
        }
        argc = n;
    }
    if (argc < 11) { fprintf(stderr, "usage: see the header of host/prove_chunk.cpp\n"); return 2; }
    const std::vector<uint64_t> program = read_words(argv[1]), trace = read_words(argv[2]), pubs = read_words(argv[3]);
    const int logn = atoi(argv[4]), logb = atoi(argv[5]), fri_logf = atoi(argv[6]), fri_final_log = atoi(argv[7]), n_queries = atoi(argv[8]),
              pow_bits = atoi(argv[9]);
    const char *air_name = argc > 11 ? argv[11] : "chunk";
    const bool sharded = argc > 14;
    const int rank = sharded ? atoi(argv[12]) : 0, world = sharded ? atoi(argv[13]) : 1;
    // the shapes must agree BEFORE anything reaches the GPU: W comes from the program header (word 1), the number of public
    // inputs from word 4; the library checks trace_words again (ZP_ERR_ARG otherwise)
    if (program.size() < 12) { fprintf(stderr, "%s: shorter than a constraint-program header\n", argv[1]); return 2; }
    const uint64_t prog_w = program[1], prog_n_pub = program[4];       // the only two header words a host needs (include/zeth_prover.h "constraint program")
    if (prog_w < 1 || prog_w >= 4096) { fprintf(stderr, "%s: width %llu out of range\n", argv[1], (unsigned long long)prog_w); return 2; }   // before it is shifted
    if (logn < 1 || logn > 30 || trace.size() != (size_t)(prog_w << logn)) {
        fprintf(stderr, "%s: %zu words, the program needs W * 2^logn = %llu * 2^%d\n", argv[2], trace.size(), (unsigned long long)prog_w, logn);
        return 2;
    }
    if (pubs.size() != prog_n_pub) { fprintf(stderr, "%s: %zu public inputs, the program declares %llu\n", argv[3], pubs.size(), (unsigned long long)prog_n_pub); return 2; }
    for (uint64_t v : trace)
        if (!check && !check_prove && v >= 0xFFFFFFFF00000001ULL) { fprintf(stderr, "%s: non-canonical trace value (precondition of zp_stark_prove)\n", argv[2]); return 2; }
    if (world < 1 || rank < 0 || rank >= world) { fprintf(stderr, "bad rank / world\n"); return 2; }
    zp_ctx *ctx = nullptr;
    uint64_t report[8];
    CHECK(zp_create(&ctx, rank));                      // one process per GPU: rank r drives device r
    // rank r owns columns [r wl, min((r + 1) wl, W)), wl = ceil(W / world): the tail ranks hold fewer columns, or none (include/zeth_prover.h)
    const size_t Wc = (size_t)prog_w, wl = (Wc + (size_t)world - 1) / (size_t)world, c0 = (size_t)rank * wl < Wc ? (size_t)rank * wl : Wc,
                 cols = Wc - c0 < wl ? Wc - c0 : wl, words = cols << logn;
    const uint64_t *mine = trace.data() + (c0 << logn);                // this rank's columns (a real host would read only these)
    void *d_trace = nullptr;
    CHECK(zp_dev_alloc(ctx, (words ? words : 1) * 8, &d_trace));
    if (words) CHECK(zp_h2d(ctx, d_trace, mine, words * 8));
    if (check && !sharded) {
        CHECK(zp_stark_check_witness(ctx, program.data(), program.size(), (const uint64_t *)d_trace, trace.size(), pubs.data(), (int32_t)pubs.size(), logn, nullptr,
                                     report, nullptr, nullptr, 0, 0));
        if (!print_report(report)) {
            if (diagnose && report[0] == ZP_WITNESS_VIOLATED) CHECK(print_diagnosis(ctx, program, d_trace, trace.size(), logn));
            zp_dev_free(ctx, d_trace);
            zp_destroy(ctx);
            return 3;
        }
    }
    char *json = nullptr;
    size_t len = 0;
    zp_comm *comm = nullptr;
    auto give_up = [&](int status) {                   // a run that ends without a proof
        if (comm) zp_comm_destroy(comm);
        zp_dev_free(ctx, d_trace);
        zp_destroy(ctx);
        return status;
    };
    if (sharded) {
        uint8_t id[128];
        const uint64_t nonce = argc > 15 ? strtoull(argv[15], nullptr, 0) : 0;
        if (rank == 0) {
            CHECK(zp_comm_unique_id(id));
            if (!zp_rendezvous::publish(argv[14], nonce, id)) { fprintf(stderr, "cannot write %s\n", argv[14]); return 2; }
        } else if (!zp_rendezvous::await(argv[14], nonce, id)) {
            fprintf(stderr, "no RCCL id of this run in %s after 60 s\n", argv[14]);
            return 2;
        }
        CHECK(zp_comm_create(ctx, rank, world, id, &comm));
        if (rank == 0) zp_rendezvous::retire(argv[14]);
        if (check) {                                   // every rank hands in its own columns and receives the report of the whole trace
            CHECK(zp_stark_check_witness_sharded(comm, program.data(), program.size(), words ? (const uint64_t *)d_trace : nullptr, words, pubs.data(),
                                                 (int32_t)pubs.size(), logn, nullptr, report, nullptr, nullptr, 0));
            if (rank == 0 ? !print_report(report) : report[0] != ZP_WITNESS_SATISFIED) return give_up(3);
        }
    }
    if (check_prove) CHECK(zp_set_tuning(ctx, "prove_check", 1));
    const int32_t rc = sharded ? zp_stark_prove_sharded(comm, air_name, program.data(), program.size(), (const uint64_t *)d_trace, words, pubs.data(),
                                                        (int32_t)pubs.size(), logn, logb, fri_logf, fri_final_log, n_queries, pow_bits, &json, &len)
                               : zp_stark_prove(ctx, air_name, program.data(), program.size(), (const uint64_t *)d_trace, trace.size(), pubs.data(),
                                                (int32_t)pubs.size(), logn, logb, fri_logf, fri_final_log, n_queries, pow_bits, &json, &len);
    if (rc != 0 && !(check_prove && rc == ZP_ERR_WITNESS)) {
        fprintf(stderr, "%s -> %d: %s\n", sharded ? "zp_stark_prove_sharded" : "zp_stark_prove", rc, zp_last_error(ctx));
        return 1;
    }
    if (check_prove) {                                 // the proof's own verdict, the same on every rank: rank 0 prints it
        CHECK(zp_stark_prove_witness_report(ctx, report, nullptr, nullptr, nullptr, (int32_t)program[8]));
        const bool refused = (rank == 0 ? !print_report(report) : report[0] != ZP_WITNESS_SATISFIED) || rc != 0;
        if (refused && diagnose && !sharded && report[0] == ZP_WITNESS_VIOLATED) CHECK(print_diagnosis(ctx, program, d_trace, trace.size(), logn));   // the prover only read the trace
        if (refused) return give_up(3);
    }
    if (rank == 0) {
        FILE *o = fopen(argv[10], "wb");
        if (!o || fwrite(json, 1, len, o) != len) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
        fclose(o);
    }
    zp_free_buffer(json);
    if (comm) zp_comm_destroy(comm);
    zp_dev_free(ctx, d_trace);
    zp_destroy(ctx);
    printf("rank %d/%d proof: %zu bytes%s%s\n", rank, world, len, rank == 0 ? " -> " : "", rank == 0 ? argv[10] : "");
    return 0;
}
