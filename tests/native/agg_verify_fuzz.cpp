// Host sanitizer driver for the aggregated-proof verifier of eigen_zeth_amd/csrc/verify.hip (built by tests/test_agg_verify_fuzz.py with
// -fsanitize=address,undefined): an aggregated proof is a TEXT a client hands in (GenFinalProof, prover.proto:130-148) -- a tree of headers, shape
// dictionaries and public inputs that size sponge streams, index tables and the batch of fixed-column evaluations.  argv: a statement table
// (host/agg_table.hpp), one good level-2 text, a count.  The text is judged as it stands (ACCEPT), then under seeded byte- and token-level mutations
// through zp_aggregate_verify(NULL, ..., ZP_VERIFY_HEADER_ONLY): every call must return ZP_OK -- a verdict, whatever it is -- and no sanitizer may fire.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../host/agg_table.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static bool read_file(const char *path, std::vector<char> *out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

// the [begin, end) of a random token: a run of digits, or one structural character
static void random_token(const std::string &t, size_t *b, size_t *e) {
    size_t at = rnd() % t.size();
    if (t[at] >= '0' && t[at] <= '9') {
        *b = at; *e = at + 1;
        while (*b > 0 && t[*b - 1] >= '0' && t[*b - 1] <= '9') (*b)--;
        while (*e < t.size() && t[*e] >= '0' && t[*e] <= '9') (*e)++;
    } else { *b = at; *e = at + 1; }
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<char> table_file, text_file;
    if (!read_file(argv[1], &table_file) || !read_file(argv[2], &text_file) || text_file.empty()) return 2;
    AggTable table;
    if (!table.load(table_file)) { printf("FAIL statement table\n"); return 1; }
    const std::string good(text_file.begin(), text_file.end());
    const long iters = atol(argv[3]);
    long verdicts[12] = {0};
    auto run = [&](const std::string &t) {
        char *buf = (char *)malloc(t.size() ? t.size() : 1);      // exactly sized, not terminated: the red zone sits right behind the text
        memcpy(buf, t.data(), t.size());
        int32_t verdict = -1, where = -2;
        const int32_t rc = zp_aggregate_verify(nullptr, table.stmts.data(), (int32_t)table.stmts.size(), buf, t.size(), ZP_VERIFY_HEADER_ONLY, 1, &verdict, &where);
        free(buf);
        if (rc != ZP_OK || verdict < 0 || verdict > 11) { printf("FAIL rc %d verdict %d on a text of %zu bytes\n", rc, verdict, t.size()); exit(1); }
        verdicts[verdict]++;
        return verdict;
    };
    if (run(good) != ZP_VERDICT_ACCEPT) { printf("FAIL the good text is not accepted\n"); return 1; }
    static const char *const tokens[] = {"0", "1", "18446744069414584321", "18446744073709551615", "99999999999999999999999", "-1", "1.5", "[]", "{}", "[[]]", "\"x\"", "null",
                                         "4096", "4097", "1073741824", ",", "]", "}", "[", "{", ":", "\"shape\"", "\"children\"", "\"inner\"", "\"queries\":[]"};
    for (long i = 0; i < iters; i++) {
        std::string t = good;
        const int kind = (int)(rnd() % 6);
        const int n_mut = 1 + (int)(rnd() % 3);
        for (int m = 0; m < n_mut && !t.empty(); m++) {
            size_t b, e;
            switch (kind) {
                case 0: t[rnd() % t.size()] = (char)(rnd() & 0xFF); break;                                   // a byte
                case 1: t.resize(rnd() % t.size()); break;                                                   // truncation
                case 2: random_token(t, &b, &e); t.replace(b, e - b, tokens[rnd() % (sizeof tokens / sizeof *tokens)]); break;      // a token replaced
                case 3: random_token(t, &b, &e); t.erase(b, e - b); break;                                   // a token dropped
                case 4: random_token(t, &b, &e); t.insert(b, tokens[rnd() % (sizeof tokens / sizeof *tokens)]); break;              // a token inserted
                default: {                                                                                    // a digit changed: stays in the grammar
                    size_t at = rnd() % t.size();
                    for (size_t k = 0; k < t.size() && !(t[at] >= '0' && t[at] <= '9'); k++) at = (at + 1) % t.size();
                    if (t[at] >= '0' && t[at] <= '9') t[at] = (char)('0' + rnd() % 10);
                }
            }
        }
        run(t);
    }
    printf("ok: %ld mutations, verdicts", iters);
    for (int v = 0; v < 12; v++) printf(" %d:%ld", v, verdicts[v]);
    printf("\n");
    return 0;
}
