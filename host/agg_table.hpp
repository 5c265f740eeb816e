// The statement-table file of an aggregated proof (written by eigen_zeth_amd/stark/agg_statements.py: write_table) -> zp_agg_statement[].
// Little-endian u64 words: "ZPAGST1\0" | n | per statement: shape_bytes (0 = the leaf statement) | shape JSON, zero padded to whole words |
// program_words | program | logn | logb | fri_logf | fri_final_log | n_queries | pow_bits | n_slots.  Every read is bounded by the file's length.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../include/zeth_prover.h"

struct AggTable {
    std::vector<uint64_t> words;               // the file; programs are used in place
    std::vector<std::string> shapes;
    std::vector<zp_agg_statement> stmts;
    bool load(const std::vector<char> &file) {
        static const char magic[8] = {'Z', 'P', 'A', 'G', 'S', 'T', '1', 0};
        if (file.size() < 16 || file.size() % 8 || memcmp(file.data(), magic, 8) != 0) return false;
        words.resize(file.size() / 8);
        memcpy(words.data(), file.data(), file.size());
        const size_t n = words.size();
        const uint64_t count = words[1];
        if (count < 1 || count > 64) return false;
        shapes.reserve(count);
        size_t at = 2;
        for (uint64_t s = 0; s < count; s++) {
            if (at >= n) return false;
            const uint64_t bytes = words[at++];
            if (bytes > (1u << 16) || (bytes + 7) / 8 > n - at) return false;
            shapes.emplace_back((const char *)&words[at], (size_t)bytes);
            at += (bytes + 7) / 8;
            if (at >= n) return false;
            const uint64_t pw = words[at++];
            if (pw > n - at || n - at - pw < 7) return false;
            zp_agg_statement st;
            st.shape_json = nullptr;
            st.h_program = &words[at];
            st.program_words = (size_t)pw;
            at += pw;
            for (int k = 0; k < 7; k++)
                if (words[at + k] > (1u << 30)) return false;
            st.logn = (int32_t)words[at]; st.logb = (int32_t)words[at + 1]; st.fri_logf = (int32_t)words[at + 2]; st.fri_final_log = (int32_t)words[at + 3];
            st.n_queries = (int32_t)words[at + 4]; st.pow_bits = (int32_t)words[at + 5]; st.n_slots = (int32_t)words[at + 6];
            at += 7;
            stmts.push_back(st);
        }
        if (at != n) return false;
        for (size_t s = 0; s < stmts.size(); s++) stmts[s].shape_json = shapes[s].empty() ? nullptr : shapes[s].c_str();      // (shapes no longer moves)
        return true;
    }
};
