// Host sanitizer driver for eigen_zeth_amd/csrc/witness_host.hip + csrc/verify.hip (built by tests/test_witness_check_fuzz.py with
// -fsanitize=address,undefined): zp_stark_check_witness with ctx = NULL.  Blob, public inputs and trace are a foreign host's: nothing of them
// may be trusted.  The file named on the command line holds a valid case
//   [program words][program][n_pubs][pubs][logn][has_chal][chal 3][trace W * 2^logn][report 8][counts K][first rows K]
// which is run as it stands (the recorded report must come back), then under seeded mutations of the blob, the public inputs, the trace, the
// trace length and logn -- every call must return ZP_OK or an error code, an error must leave the outputs as they were, and no sanitizer may fire.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int32_t zp_stark_check_witness(void *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words,
                                          const uint64_t *h_pubs, int32_t n_pubs, int32_t logn, const uint64_t *h_chal3, uint64_t *h_report,
                                          uint64_t *h_counts, uint64_t *h_first_row, int32_t n_constraints, int32_t threads);

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> all;
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) all.push_back(w);
    fclose(f);
    size_t at = 0;
    auto take = [&](size_t n) { const uint64_t *p = all.data() + at; at += n; return std::vector<uint64_t>(p, p + n); };
    const size_t pw = (size_t)take(1)[0];
    const std::vector<uint64_t> prog = take(pw);
    const size_t np = (size_t)take(1)[0];
    const std::vector<uint64_t> pubs = take(np);
    const int logn = (int)take(1)[0];
    const bool has_chal = take(1)[0] != 0;
    const std::vector<uint64_t> chal = take(3);
    const size_t W = (size_t)prog[1], K = (size_t)prog[8];
    const std::vector<uint64_t> trace = take(W << logn), want_rep = take(8), want_counts = take(K), want_first = take(K);
    if (at != all.size()) { printf("FAIL case file\n"); return 1; }
    const uint64_t MARK = 0x5A5A5A5A5A5A5A5AULL;
    // exactly-sized heap buffers: the red zones sit right behind them.  The caller's arrays keep THEIR sizes (K counts, K first rows, the trace as
    // long as it says): a mutated header that names other sizes must be refused
    auto run = [&](const std::vector<uint64_t> &p, const std::vector<uint64_t> &pb, const std::vector<uint64_t> &tr, int lg, int threads, std::vector<uint64_t> *out) {
        uint64_t *pp = (uint64_t *)malloc(p.size() * 8 + 8), *pbp = (uint64_t *)malloc(pb.size() * 8 + 8), *t = (uint64_t *)malloc(tr.size() * 8 + 8);
        uint64_t *o = (uint64_t *)malloc((8 + 2 * K) * 8);
        memcpy(pp, p.data(), p.size() * 8); memcpy(pbp, pb.data(), pb.size() * 8); memcpy(t, tr.data(), tr.size() * 8);
        for (size_t i = 0; i < 8 + 2 * K; i++) o[i] = MARK;
        const int32_t rc = zp_stark_check_witness(nullptr, pp, p.size(), t, tr.size(), pbp, (int32_t)pb.size(), lg, has_chal ? chal.data() : nullptr, o, o + 8, o + 8 + K,
                                                  (int32_t)K, threads);
        bool touched = false;
        for (size_t i = 0; i < 8 + 2 * K; i++) touched |= o[i] != MARK;
        if (rc != 0 && touched) { printf("FAIL outputs written on an error\n"); exit(1); }
        if (rc == 0 && memcmp(t, tr.data(), tr.size() * 8) != 0) { printf("FAIL the trace was written\n"); exit(1); }
        if (out && rc == 0) out->assign(o, o + 8 + 2 * K);
        free(pp); free(pbp); free(t); free(o);
        return rc;
    };
    std::vector<uint64_t> got, want = want_rep;
    want.insert(want.end(), want_counts.begin(), want_counts.end());
    want.insert(want.end(), want_first.begin(), want_first.end());
    for (int threads : {1, 3})
        if (run(prog, pubs, trace, logn, threads, &got) != 0 || got != want) { printf("FAIL the valid case\n"); return 1; }
    uint64_t s = 0x2545F4914F6CDD1DULL;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    int ok = 0, refused = 0;
    const int iters = argc > 2 ? atoi(argv[2]) : 3000;
    for (int it = 0; it < iters; it++) {
        std::vector<uint64_t> p = prog, pb = pubs, tr = trace;
        int lg = logn;
        const int n_mut = 1 + (int)(rnd() % 3);
        for (int m = 0; m < n_mut; m++) {
            switch (rnd() % 11) {
            case 0: p[rnd() % 12] = rnd() % 5000; break;                                   // a header field
            case 1: p[rnd() % 12] = rnd(); break;
            case 2: p[12 + rnd() % (p.size() - 12)] = rnd(); break;                        // anything behind it
            case 3: p[12 + rnd() % (p.size() - 12)] ^= 1ULL << (rnd() % 64); break;
            case 4: p.resize(12 + rnd() % (p.size() - 12)); break;                         // truncated
            case 5: if (!pb.empty()) pb[rnd() % pb.size()] = rnd(); break;
            case 6: pb.resize(rnd() % (pb.size() + 2)); break;
            case 7: tr[rnd() % tr.size()] = rnd(); break;                                  // mostly canonical, sometimes >= p
            case 8: tr.resize(1 + rnd() % (2 * tr.size())); break;                         // a trace of another length
            case 9: { const int d = (int)(rnd() % 3) - 1; lg += d; if (d > 0) tr.resize(tr.size() * 2); if (d < 0) tr.resize(tr.size() / 2 ? tr.size() / 2 : 1); break; }
            default: lg = (int)(rnd() % 40) - 2; break;
            }
            if (p.size() < 13) break;
        }
        const int32_t rc = run(p, pb, tr, lg, 1 + it % 3, nullptr);
        if (rc == 0) ok++; else refused++;
    }
    printf("ok: %d mutated cases judged, %d refused\n", ok, refused);
    return 0;
}
