// The constraint check's result words and what is made of them -- HOST code only, plain C++ (tests/native/witness_merge_check.cpp builds it under
// the host sanitizers).  A result is [first (row << 24 | k) key][first_row: K][counts: K] (csrc/witness_check.hip: what the kernels write);
// zpi_witness_report is the ONE place the 8-word report of zp_stark_check_witness is made from it, for one GPU and for the ranks of a communicator.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/zeth_prover.h"

inline size_t zpi_witness_result_words(size_t K) { return 1 + 2 * K; }

// G results, one after the other (what an all-gather of every rank's result delivers) -> one: counts summed, the first rows and the first key lowered.
// Ranks judge disjoint row windows, so a sum counts no (row, constraint) pair twice.
inline void zpi_witness_merge(const uint64_t *parts, size_t G, size_t K, uint64_t *out) {
    const size_t words = zpi_witness_result_words(K);
    memset(out, 0xFF, (1 + K) * 8);
    memset(out + 1 + K, 0, K * 8);
    for (size_t g = 0; g < G; g++) {
        const uint64_t *p = parts + g * words;
        if (p[0] < out[0]) out[0] = p[0];
        for (size_t k = 0; k < K; k++) {
            if (p[1 + k] < out[1 + k]) out[1 + k] = p[1 + k];
            out[1 + K + k] += p[1 + K + k];
        }
    }
}

// the report of a result (h_counts / h_first_row: K words each, or NULL)
inline void zpi_witness_report(const uint64_t *res, size_t K, uint64_t *h_report, uint64_t *h_counts, uint64_t *h_first_row) {
    uint64_t rep[8] = {ZP_WITNESS_SATISFIED, ~0ULL, ~0ULL, 0, 0, 0, ~0ULL, ~0ULL};
    const uint64_t *first = res + 1, *counts = first + K;
    for (size_t k = 0; k < K; k++) { rep[3] += counts[k]; rep[4] += counts[k] != 0; }
    if (rep[3]) {
        rep[0] = ZP_WITNESS_VIOLATED;
        rep[1] = res[0] >> 24;
        rep[2] = res[0] & 0xFFFFFF;
    }
    memcpy(h_report, rep, sizeof rep);
    if (h_counts) memcpy(h_counts, counts, K * 8);
    if (h_first_row) memcpy(h_first_row, first, K * 8);
}
