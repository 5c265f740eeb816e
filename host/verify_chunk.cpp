// A compiled host above the C-ABI that CHECKS a chunk proof: what a Rust prover service does with a proof text a client hands in before it
// aggregates it.  Nothing but include/zeth_prover.h is used -- no Python, no torch (the statement is a data blob, the proof a text file).
//
// usage: verify_chunk <program.bin> <proof.json> <logn> <logb> <fri_logf> <fri_final_log> <n_queries> <pow_bits> [host]
//   program.bin : the constraint program blob (u64 words, layout in the header)
//   proof.json  : the text zp_stark_prove / host/prove_chunk wrote
//   host        : verify without a GPU (ctx = NULL: default tables and domain)
//        verify_chunk aggregated <statements.bin> <aggregated.json> [host] [header-only]
//   statements.bin : the statement table of the text's shapes (eigen_zeth_amd/stark/agg_statements.py: write_table; layout in host/agg_table.hpp) --
//                    the chunk AIR's program and, per shape of the tree, the verifier AIR's program with the verifier's parameters
//   aggregated.json: what GenAggregatedProof returned (any level); judged by zp_aggregate_verify
//   header-only    : skip the outer STARK's openings (ZP_VERIFY_HEADER_ONLY: a final STARK over the text proves them)
// prints "verdict <code> <name> where <query / node or -1>"; exit status 0 = accepted, 1 = rejected, 2 = could not be checked
// build: make -C host
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/zeth_prover.h"
#include "agg_table.hpp"

static bool read_file(const char *path, std::string *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
    fclose(f);
    return true;
}

static const char *const verdict_names[] = {"accept", "malformed", "params", "identity", "pow", "indices", "final-degree", "opening", "fri", "transcript", "publics", "tree"};

static int aggregated_main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: see the header of host/verify_chunk.cpp\n"); return 2; }
    std::string table_file, text;
    if (!read_file(argv[2], &table_file) || !read_file(argv[3], &text)) { fprintf(stderr, "cannot read %s / %s\n", argv[2], argv[3]); return 2; }
    AggTable table;
    if (!table.load(std::vector<char>(table_file.begin(), table_file.end()))) { fprintf(stderr, "%s is no statement table\n", argv[2]); return 2; }
    bool on_host = false;
    uint32_t flags = 0;
    for (int i = 4; i < argc; i++) {
        if (!strcmp(argv[i], "host")) on_host = true;
        else if (!strcmp(argv[i], "header-only")) flags |= ZP_VERIFY_HEADER_ONLY;
    }
    zp_ctx *ctx = nullptr;
    if (!on_host && zp_create(&ctx, 0) != ZP_OK) { fprintf(stderr, "zp_create failed: no GPU? (pass `host` to verify without one)\n"); return 2; }
    int32_t verdict = ZP_VERDICT_MALFORMED, where = -1;
    const int32_t rc = zp_aggregate_verify(ctx, table.stmts.data(), (int32_t)table.stmts.size(), text.data(), text.size(), flags, 0, &verdict, &where);
    if (rc != ZP_OK) fprintf(stderr, "zp_aggregate_verify -> %d: %s\n", rc, ctx ? zp_last_error(ctx) : "bad arguments");
    if (ctx) zp_destroy(ctx);
    if (rc != ZP_OK) return 2;
    printf("verdict %d %s where %d\n", verdict, verdict >= 0 && verdict <= 11 ? verdict_names[verdict] : "?", where);
    return verdict == ZP_VERDICT_ACCEPT ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "aggregated")) return aggregated_main(argc, argv);
    if (argc < 9) { fprintf(stderr, "usage: see the header of host/verify_chunk.cpp\n"); return 2; }
    std::string blob, text;
    if (!read_file(argv[1], &blob) || blob.size() % 8 || !read_file(argv[2], &text)) { fprintf(stderr, "cannot read %s / %s\n", argv[1], argv[2]); return 2; }
    std::vector<uint64_t> program(blob.size() / 8);
    memcpy(program.data(), blob.data(), blob.size());
    const bool on_host = argc > 9 && !strcmp(argv[9], "host");
    zp_ctx *ctx = nullptr;
    if (!on_host && zp_create(&ctx, 0) != ZP_OK) { fprintf(stderr, "zp_create failed: no GPU? (pass `host` to verify without one)\n"); return 2; }
    int32_t verdict = ZP_VERDICT_MALFORMED, where = -1;
    const int32_t rc = zp_stark_verify(ctx, program.data(), program.size(), text.data(), text.size(), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]),
                                       atoi(argv[7]), atoi(argv[8]), 0, 0, &verdict, &where, nullptr);
    if (rc != ZP_OK) fprintf(stderr, "zp_stark_verify -> %d: %s\n", rc, ctx ? zp_last_error(ctx) : "bad arguments");
    if (ctx) zp_destroy(ctx);
    if (rc != ZP_OK) return 2;
    printf("verdict %d %s where %d\n", verdict, verdict >= 0 && verdict <= 8 ? verdict_names[verdict] : "?", where);
    return verdict == ZP_VERDICT_ACCEPT ? 0 : 1;
}
