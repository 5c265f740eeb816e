// Host sanitizer driver for the BN128-hash mode of the STARK verifier (eigen_zeth_amd/csrc/verify.hip + proofparse.hip, built by
// tests/test_stark_verify_bn128_host.py with -fsanitize=address,undefined and linked with nothing else): the final STARK's TEXT comes from a client
// and reaches zp_stark_verify_bn128 through a C ABI, so nothing in it may be trusted -- least of all the length of a quoted field element.
// usage: stark_verify_bn128_fuzz <program.bin> <proof.json> <tables.bin> <rp> <logn> <logb> <fri_logf> <fri_final_log> <n_queries> <iterations>
//   tables.bin: the t = 17 Poseidon-BN254 tables, (8 + rp) * 17 round constants then 17 * 17 matrix entries, four little-endian words each
// The valid text is verified as it stands (must be accepted, ctx = NULL: everything on the host), then under seeded mutations -- bytes overwritten,
// inserted and deleted, the text cut short, a closing quote removed, a number (quoted or not) replaced by another one (small, near p, near r, near
// 2^256, very long, with a leading zero, with a sign), now and then a mutated program blob or flags: every call must end in a verdict or an error
// code, and no sanitizer may fire.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int32_t zp_stark_verify_bn128(void *ctx, const uint64_t *h_program, size_t program_words, const char *proof_json, size_t proof_len, int32_t logn, int32_t logb,
                                         int32_t fri_logf, int32_t fri_final_log, int32_t n_queries, int32_t rp, const uint64_t *h_rc, const uint64_t *h_mds, uint32_t flags,
                                         int32_t threads, int32_t *verdict, int32_t *where, uint64_t *h_indices);

static std::string read_all(const char *path) {
    std::string s;
    FILE *f = fopen(path, "rb");
    if (!f) return s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

int main(int argc, char **argv) {
    if (argc < 11) return 2;
    const std::string blob = read_all(argv[1]), text = read_all(argv[2]), tab = read_all(argv[3]);
    const int rp = atoi(argv[4]);
    int a[5];
    for (int i = 0; i < 5; i++) a[i] = atoi(argv[5 + i]);
    const int iters = atoi(argv[10]);
    const size_t nrc = (size_t)(8 + rp) * 17 * 4, nm = 17 * 17 * 4;
    if (blob.empty() || blob.size() % 8 || text.empty() || rp < 1 || tab.size() != (nrc + nm) * 8) { printf("FAIL case files\n"); return 1; }
    std::vector<uint64_t> prog(blob.size() / 8), tables(nrc + nm);
    memcpy(prog.data(), blob.data(), blob.size());
    memcpy(tables.data(), tab.data(), tab.size());
    // exactly-sized heap copies: the red zones sit right behind the text, the blob, the tables and the index array
    auto run = [&](const std::vector<uint64_t> &p, const std::string &t, uint32_t flags, int32_t *verdict) {
        uint64_t *pp = (uint64_t *)malloc(p.size() * 8 + 1);
        char *tt = (char *)malloc(t.size() + 1);
        uint64_t *idx = (uint64_t *)malloc((size_t)a[4] * 8);
        uint64_t *tb = (uint64_t *)malloc(tables.size() * 8);
        memcpy(pp, p.data(), p.size() * 8);
        memcpy(tt, t.data(), t.size());
        memcpy(tb, tables.data(), tables.size() * 8);
        int32_t where = -1;
        const int32_t rc = zp_stark_verify_bn128(nullptr, pp, p.size(), tt, t.size(), a[0], a[1], a[2], a[3], a[4], rp, tb, tb + nrc, flags, 8, verdict, &where, idx);
        free(pp); free(tt); free(idx); free(tb);
        return rc;
    };
    int32_t verdict = -1;
    if (run(prog, text, 0, &verdict) != 0 || verdict != 0) { printf("FAIL the valid case: verdict %d\n", verdict); return 1; }
    uint64_t s = 0x2545F4914F6CDD1DULL;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    const std::string r_dec = "21888242871839275222246405745257275088548364400416034343698204186575808495617";
    const std::string two256 = "115792089237316195423570985008687907853269984665640564039457584007913129639936";
    const std::vector<std::string> numbers = {"0", "1", "18446744069414584320", "18446744069414584321", "18446744073709551615", "18446744073709551616",
                                              r_dec, r_dec.substr(0, r_dec.size() - 1) + "6", two256, two256.substr(0, two256.size() - 1) + "5",
                                              std::string(300, '9'), std::string(70000, '7'), "00", "017", "-1", "+5", "1.5", "1e3", ""};
    static const char junk[] = "{}[],:\"0 9-e\\\n";
    int verdicts[9] = {0}, errors = 0;
    for (int it = 0; it < iters; it++) {
        std::string t = text;
        std::vector<uint64_t> p = prog;
        uint32_t flags = rnd() % 8 == 0 ? (uint32_t)(rnd() % 4) : 0;
        const int n_mut = 1 + (int)(rnd() % 3);
        for (int m = 0; m < n_mut && !t.empty(); m++) {
            const size_t at = (size_t)(rnd() % t.size());
            switch (rnd() % 9) {
                case 0: t[at] = junk[rnd() % (sizeof junk - 1)]; break;
                case 1: t[at] = (char)(rnd() & 0xFF); break;
                case 2: t.insert(at, 1, junk[rnd() % (sizeof junk - 1)]); break;
                case 3: t.erase(at, 1 + (size_t)(rnd() % 4)); break;
                case 4: t.resize(at); break;
                case 5: p[(size_t)(rnd() % p.size())] = rnd() % 4 ? rnd() % 64 : rnd(); break;
                case 6: {                                    // the next closing quote goes: an unterminated string
                    const size_t qd = t.find("\",", at);
                    if (qd != std::string::npos) t.erase(qd, 1);
                    break;
                }
                default: {                                   // the number at or behind `at`, quoted or not, becomes another number
                    size_t b = at;
                    while (b < t.size() && (t[b] < '0' || t[b] > '9')) b++;
                    while (b > 0 && t[b - 1] >= '0' && t[b - 1] <= '9') b--;
                    size_t e = b;
                    while (e < t.size() && t[e] >= '0' && t[e] <= '9') e++;
                    if (e > b) t.replace(b, e - b, numbers[rnd() % numbers.size()]);
                }
            }
        }
        verdict = -1;
        const int32_t rc = run(p, t, flags, &verdict);
        if (rc == 0 && verdict >= 0 && verdict <= 8) verdicts[verdict]++;
        else if (rc < 0) errors++;
        else { printf("FAIL iteration %d: rc %d verdict %d\n", it, rc, verdict); return 1; }
    }
    printf("ok: %d mutations; verdicts", iters);
    for (int v = 0; v < 9; v++) printf(" %d", verdicts[v]);
    printf("; error codes %d\n", errors);
    return 0;
}
