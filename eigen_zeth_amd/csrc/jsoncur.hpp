// The strict cursor over a proof text that csrc/proofparse.hip (the query openings) and csrc/verify.hip (the header) read with: host code,
// no allocation, every read bounded by `end`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace zpjson {

struct Cur {
    const char *p, *end;
    bool ok = true;
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
    bool eat(char c) {
        ws();
        if (p < end && *p == c) { p++; return true; }
        return false;
    }
    bool need(char c) {
        if (!eat(c)) ok = false;
        return ok;
    }
    bool peek(char c) { ws(); return p < end && *p == c; }
    // a JSON string without escapes we care about: returns [b, e) of its content
    bool str(const char **b, const char **e) {
        ws();
        if (p >= end || *p != '"') { ok = false; return false; }
        p++;
        *b = p;
        while (p < end && *p != '"') {
            if (*p == '\\') { p++; if (p >= end) break; }
            p++;
        }
        if (p >= end) { ok = false; return false; }
        *e = p;
        p++;
        return true;
    }
    bool key_is(const char *b, const char *e, const char *k) { return (size_t)(e - b) == strlen(k) && memcmp(b, k, e - b) == 0; }
    bool u64v(uint64_t *out) {                 // non-negative decimal integer < 2^64
        ws();
        if (p >= end || *p < '0' || *p > '9') { ok = false; return false; }
        uint64_t v = 0;
        int digits = 0;
        while (p < end && *p >= '0' && *p <= '9') {
            const unsigned d = (unsigned)(*p - '0');
            if (v > (UINT64_MAX - d) / 10) { ok = false; return false; }
            v = v * 10 + d;
            p++;
            digits++;
        }
        if (p < end && (*p == '.' || *p == 'e' || *p == 'E')) { ok = false; return false; }
        *out = v;
        return digits > 0;
    }
    // a field element of a BN128-mode text: a QUOTED decimal in the strict grammar its prover writes (one or more digits, no sign, no leading
    // zero except "0") into four little-endian words.  A string of any length is read to its end: a value >= 2^256 becomes all ones, which
    // is >= r and so equals nothing
    bool dec256(uint64_t w[4]) {
        ws();
        if (p >= end || *p != '"') { ok = false; return false; }
        const char *b = ++p;
        bool over = false;
        w[0] = w[1] = w[2] = w[3] = 0;
        for (; p < end && *p >= '0' && *p <= '9'; p++) {
            unsigned __int128 c = (unsigned)(*p - '0');
            for (int k = 0; k < 4; k++) { c += (unsigned __int128)w[k] * 10; w[k] = (uint64_t)c; c >>= 64; }
            over |= c != 0;
        }
        if (p == b || (p - b > 1 && *b == '0') || p >= end || *p != '"') { ok = false; return false; }
        p++;
        if (over) w[0] = w[1] = w[2] = w[3] = ~(uint64_t)0;
        return true;
    }
    void skip_value(int depth = 0) {          // any JSON value
        ws();
        if (!ok || p >= end || depth > 64) { ok = false; return; }
        if (*p == '"') { const char *b, *e; str(&b, &e); return; }
        if (*p == '{' || *p == '[') {
            const char close = *p == '{' ? '}' : ']';
            const bool obj = *p == '{';
            p++;
            if (eat(close)) return;
            for (;;) {
                if (obj) { const char *b, *e; if (!str(&b, &e) || !need(':')) return; }
                skip_value(depth + 1);
                if (!ok) return;
                if (eat(',')) continue;
                need(close);
                return;
            }
        }
        const char *q = p;                    // number / true / false / null
        while (p < end && *p != ',' && *p != '}' && *p != ']' && *p != ' ' && *p != '\n' && *p != '\t' && *p != '\r') p++;
        if (p == q) ok = false;
    }
};

// walks the members of the object at c; calls f(key begin, key end) positioned at the value; f must consume the value
template <typename F>
bool each_member(Cur &c, F f) {
    if (!c.need('{')) return false;
    if (c.eat('}')) return true;
    for (;;) {
        const char *b, *e;
        if (!c.str(&b, &e) || !c.need(':')) return false;
        f(b, e);
        if (!c.ok) return false;
        if (c.eat(',')) continue;
        return c.need('}');
    }
}

}  // namespace zpjson
