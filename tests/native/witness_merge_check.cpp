// csrc/witness_merge.hpp under the host sanitizers: hand-made per-rank results [first key][first_row: K][counts: K] through zpi_witness_merge and
// zpi_witness_report.  A stand-alone program (tests/test_witness_merge_host.py builds and runs it); prints "ok" and exits 0 when every case holds.
#include <cstdio>
#include <vector>

#include "../../eigen_zeth_amd/csrc/witness_merge.hpp"

typedef uint64_t u64;
static const u64 NONE = ~0ULL;
static int failures = 0;

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

// a rank's result from its violated (row, constraint) pairs, as the kernels would leave it
static std::vector<u64> result(size_t K, const std::vector<std::pair<u64, u64>> &pairs) {
    std::vector<u64> r(zpi_witness_result_words(K), 0);
    for (size_t i = 0; i <= K; i++) r[i] = NONE;
    for (const auto &p : pairs) {
        const u64 key = (p.first << 24) | p.second;
        if (key < r[0]) r[0] = key;
        if (p.first < r[1 + p.second]) r[1 + p.second] = p.first;
        r[1 + K + p.second]++;
    }
    return r;
}

static std::vector<u64> gathered(const std::vector<std::vector<u64>> &ranks) {
    std::vector<u64> all;
    for (const auto &r : ranks) all.insert(all.end(), r.begin(), r.end());
    return all;
}

int main() {
    {   // all empty, over 1, 2 and 8 ranks: satisfied, nothing to name
        for (size_t G : {1, 2, 8}) {
            const size_t K = 5;
            const std::vector<u64> all = gathered(std::vector<std::vector<u64>>(G, result(K, {})));
            std::vector<u64> m(zpi_witness_result_words(K)), counts(K, 7), first(K, 7);
            u64 rep[8];
            zpi_witness_merge(all.data(), G, K, m.data());
            zpi_witness_report(m.data(), K, rep, counts.data(), first.data());
            EXPECT(rep[0] == ZP_WITNESS_SATISFIED && rep[1] == NONE && rep[2] == NONE && rep[3] == 0 && rep[4] == 0 && rep[5] == 0 && rep[6] == NONE && rep[7] == NONE);
            for (size_t k = 0; k < K; k++) EXPECT(counts[k] == 0 && first[k] == NONE);
        }
    }
    {   // one rank of four violated: its result is the merged one
        const size_t K = 3;
        const std::vector<u64> mine = result(K, {{130, 2}, {129, 2}, {140, 0}});
        const std::vector<u64> all = gathered({result(K, {}), result(K, {}), mine, result(K, {})});
        std::vector<u64> m(zpi_witness_result_words(K));
        u64 rep[8];
        zpi_witness_merge(all.data(), 4, K, m.data());
        EXPECT(m == mine);
        zpi_witness_report(m.data(), K, rep, nullptr, nullptr);       // NULL arrays are allowed
        EXPECT(rep[0] == ZP_WITNESS_VIOLATED && rep[1] == 129 && rep[2] == 2 && rep[3] == 3 && rep[4] == 2);
    }
    {   // ties on the first row: two constraints at the smallest row on one rank (the smaller index wins); the same constraint on two ranks
        const size_t K = 4;
        const std::vector<u64> all = gathered({result(K, {{9, 3}, {9, 1}, {40, 0}}), result(K, {{70, 1}, {64, 3}, {64, 0}})});
        std::vector<u64> m(zpi_witness_result_words(K)), counts(K), first(K);
        u64 rep[8];
        zpi_witness_merge(all.data(), 2, K, m.data());
        zpi_witness_report(m.data(), K, rep, counts.data(), first.data());
        EXPECT(rep[0] == ZP_WITNESS_VIOLATED && rep[1] == 9 && rep[2] == 1 && rep[3] == 6 && rep[4] == 3);
        EXPECT(counts == (std::vector<u64>{2, 2, 0, 2}) && first == (std::vector<u64>{40, 9, NONE, 9}));
    }
    {   // the largest row and constraint a key holds, a window a rank judged last: row 2^30 - 1, constraint 2^24 - 1 of K = 2^24 is out of a test's
        // reach, so K = 2 with the largest row; and K = 0 (a program without constraints) touches nothing
        const size_t K = 2;
        const u64 top = (1ULL << 30) - 1;
        const std::vector<u64> all = gathered({result(K, {}), result(K, {{top, 1}})});
        std::vector<u64> m(zpi_witness_result_words(K));
        u64 rep[8];
        zpi_witness_merge(all.data(), 2, K, m.data());
        zpi_witness_report(m.data(), K, rep, nullptr, nullptr);
        EXPECT(rep[1] == top && rep[2] == 1 && rep[3] == 1);
        const u64 none[2] = {NONE, NONE};
        u64 m0[1] = {5};
        zpi_witness_merge(none, 2, 0, m0);
        zpi_witness_report(m0, 0, rep, nullptr, nullptr);
        EXPECT(m0[0] == NONE && rep[0] == ZP_WITNESS_SATISFIED);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
