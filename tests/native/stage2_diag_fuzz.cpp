// Host sanitizer driver for eigen_zeth_amd/csrc/stage2_diag_host.hip (built by tests/test_stage2_diag_fuzz.py with -fsanitize=address,undefined):
// zp_stark_diagnose_stage2 with ctx = NULL.  Blob and trace are a foreign host's: nothing of them may be trusted.  The file named on the command
// line holds a valid case
//   [program words][program][logn][trace W * 2^logn][records n_stage2 * 12]
// which is run as it stands (the recorded records must come back, on one thread and on three), then under seeded mutations of the blob, the
// trace, the trace length, logn and n_stage2 -- every call must return ZP_OK or ZP_ERR_ARG, an error must leave the output as it was, the trace is
// never written, and no sanitizer may fire.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int32_t zp_stark_diagnose_stage2(void *ctx, const uint64_t *h_program, size_t program_words, const uint64_t *trace, size_t trace_words, int32_t logn,
                                            uint64_t *h_diag, int32_t n_stage2, int32_t threads);

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
    const int logn = (int)take(1)[0];
    const size_t W = (size_t)prog[1], S = (size_t)prog[10];
    const std::vector<uint64_t> trace = take(W << logn), want = take(S * 12);
    if (at != all.size() || S == 0) { printf("FAIL case file\n"); return 1; }
    const uint64_t MARK = 0x5A5A5A5A5A5A5A5AULL;
    // exactly-sized heap buffers: the red zones sit right behind them.  The caller's output keeps ITS size (S records) and the trace is as long as it
    // says: a mutated header that names other sizes must be refused
    auto run = [&](const std::vector<uint64_t> &p, const std::vector<uint64_t> &tr, int lg, int n_s2, int threads, std::vector<uint64_t> *out) {
        uint64_t *pp = (uint64_t *)malloc(p.size() * 8 + 8), *t = (uint64_t *)malloc(tr.size() * 8 + 8), *o = (uint64_t *)malloc(S * 12 * 8);
        if (!p.empty()) memcpy(pp, p.data(), p.size() * 8);
        if (!tr.empty()) memcpy(t, tr.data(), tr.size() * 8);
        for (size_t i = 0; i < S * 12; i++) o[i] = MARK;
        const int32_t rc = zp_stark_diagnose_stage2(nullptr, pp, p.size(), t, tr.size(), lg, o, n_s2, threads);
        bool touched = false;
        for (size_t i = 0; i < S * 12; i++) touched |= o[i] != MARK;
        if (rc != 0 && rc != -1) { printf("FAIL return code %d\n", rc); exit(1); }
        if (rc != 0 && touched) { printf("FAIL output written on an error\n"); exit(1); }
        if (!tr.empty() && memcmp(t, tr.data(), tr.size() * 8) != 0) { printf("FAIL the trace was written\n"); exit(1); }
        if (out && rc == 0) out->assign(o, o + S * 12);
        free(pp); free(t); free(o);
        return rc;
    };
    std::vector<uint64_t> got;
    for (int threads : {1, 3})
        if (run(prog, trace, logn, (int)S, threads, &got) != 0 || got != want) { printf("FAIL the valid case\n"); return 1; }
    // short and odd buffers around the valid case
    for (size_t words : {(size_t)0, (size_t)1, trace.size() - 1, trace.size() / 2, trace.size() + 1}) {
        std::vector<uint64_t> tr = trace;
        tr.resize(words);
        if (run(prog, tr, logn, (int)S, 1, nullptr) == 0) { printf("FAIL a trace of another length was judged\n"); return 1; }
    }
    for (size_t words = 0; words < prog.size(); words += 1 + words / 7)
        if (run(std::vector<uint64_t>(prog.begin(), prog.begin() + words), trace, logn, (int)S, 1, nullptr) == 0) { printf("FAIL a cut blob was judged\n"); return 1; }
    uint64_t s = 0x2545F4914F6CDD1DULL;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    int ok = 0, refused = 0;
    const int iters = argc > 2 ? atoi(argv[2]) : 3000;
    for (int it = 0; it < iters; it++) {
        std::vector<uint64_t> p = prog, tr = trace;
        int lg = logn, n_s2 = (int)S;
        const int n_mut = 1 + (int)(rnd() % 3);
        for (int m = 0; m < n_mut; m++) {
            switch (rnd() % 11) {
            case 0: p[rnd() % 12] = rnd() % 5000; break;                                   // a header field
            case 1: p[rnd() % 12] = rnd(); break;
            case 2: p[12 + rnd() % (p.size() - 12)] = rnd(); break;                        // anything behind it
            case 3: p[12 + rnd() % (p.size() - 12)] ^= 1ULL << (rnd() % 64); break;
            case 4: p.resize(12 + rnd() % (p.size() - 12)); break;                         // truncated
            case 5: { const size_t tab = 12 + (size_t)prog[6] + (size_t)prog[7]; if (tab + 4 * S <= p.size()) p[tab + rnd() % (4 * S)] = rnd() % (2 * W); break; }   // a stage-2 entry
            case 6: tr[rnd() % tr.size()] = rnd() % 7 ? rnd() % 5 : rnd(); break;          // a small value (collides with others), sometimes >= p
            case 7: { const size_t c = rnd() % W, n = tr.size() / W; if (n) for (size_t i = 0; i < n; i++) tr[c * n + i] = rnd() % 3; break; }       // a hot column
            case 8: tr.resize(1 + rnd() % (2 * tr.size())); break;                         // a trace of another length
            case 9: { const int d = (int)(rnd() % 3) - 1; lg += d; if (d > 0) tr.resize(tr.size() * 2); if (d < 0) tr.resize(tr.size() / 2 ? tr.size() / 2 : 1); break; }
            default: if (rnd() & 1) lg = (int)(rnd() % 40) - 2; else n_s2 = (int)(rnd() % (S + 2)) - 1; break;      // never more than the output holds
            }
            if (p.size() < 13) break;
        }
        const int32_t rc = run(p, tr, lg, n_s2, 1 + it % 3, nullptr);
        if (rc == 0) ok++; else refused++;
    }
    printf("ok: %d mutated cases judged, %d refused\n", ok, refused);
    return 0;
}
