// A compiled host above the C-ABI that CHECKS a chunk proof: what a Rust prover service does with a proof text a client hands in before it
// aggregates it.  Nothing but include/zeth_prover.h is used -- no Python, no torch (the statement is a data blob, the proof a text file).
//
// usage: verify_chunk <program.bin> <proof.json> <logn> <logb> <fri_logf> <fri_final_log> <n_queries> <pow_bits> [host]
//   program.bin : the constraint program blob (u64 words, layout in the header)
//   proof.json  : the text zp_stark_prove / host/prove_chunk wrote
//   host        : verify without a GPU (ctx = NULL: default tables and domain)
// prints "verdict <code> <name> where <query or -1>"; exit status 0 = accepted, 1 = rejected, 2 = could not be checked
// build: make -C host
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/zeth_prover.h"

static bool read_file(const char *path, std::string *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
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
    static const char *const names[] = {"accept", "malformed", "params", "identity", "pow", "indices", "final-degree", "opening", "fri"};
    printf("verdict %d %s where %d\n", verdict, verdict >= 0 && verdict <= 8 ? names[verdict] : "?", where);
    return verdict == ZP_VERDICT_ACCEPT ? 0 : 1;
}
