// LDS slot addresses of the NTT pass kernels, every case (tests/test_ntt_slots.py builds and runs this; no GPU, nothing preloaded).
// For every shape dispatch_pass builds, every round, every odd j0inv in 1..15, every lane of the workgroup and every register:
//   * the factored write address of csrc/ntt_geo.hpp, (lane ^ x) + y and lane ^ (x | y), equals 8 lpos(slot_of(o, k_j, pos, A), t)
//     (shapes with the extra slot swizzle keep lpos in the kernels: for them only the permutation below is checked);
//   * a round's writes are a permutation of the tile;
//   * the copy-out read address, lane ^ constant, equals 8 lpos(sigma_of_k(k), t2), and the reads are a permutation of the tile.
// Prints one line per shape and "ok: <cases>"; the first mismatch is printed and ends the run with status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_geo.hpp"

static long long g_cases = 0;

[[noreturn]] static void fail(const char *what, int a1, int a2, int a3, int logt, int pos, int j0inv, int tid, int reg, long long got, long long want) {
    std::printf("MISMATCH %s: shape (%d,%d,%d,%d) field at %d j0inv %d lane %d register %d: %lld, lpos gives %lld\n", what, a1, a2, a3, logt, pos, j0inv, tid, reg, got, want);
    std::exit(1);
}

// one round of a tile step: the field of 2^A values at bit `pos`; `last`: the post-round write of a first pass, k_j = jr i
template <typename G>
static void check_round(int a1, int a2, int a3, int pos, int A, bool last) {
    const int GR = 16 >> A, mask = (1 << A) - 1;
    std::vector<unsigned char> seen((size_t)G::R * G::T);
    for (int j0inv = 1; j0inv < 16; j0inv += 2) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int tid = 0; tid < G::NT; tid++)
            for (int g = 0; g < GR; g++) {
                const int gamma = g * G::NT + tid;
                const int t = gamma & (G::T - 1), o = gamma >> G::LT;
                const int lane = G::wr_lane(o, t, pos, A);
                for (int p = 0; p < (1 << A); p++) {
                    const int kj = last ? ((j0inv & mask) * p) & mask : (j0inv * brev(p, A)) & mask;
                    const int want = G::lpos(slot_of(o, kj, pos, A), t);
                    if constexpr (G::FACTORED) {
                        const int x = G::wr_xor(kj, pos, A), y = G::wr_add(kj, pos, A);
                        if (G::wr_pos(lane, x, y) != 8 * want) fail("(lane ^ x) + y", a1, a2, a3, G::LT, pos, j0inv, tid, g * (1 << A) + p, G::wr_pos(lane, x, y), 8LL * want);
                        if ((lane ^ G::wr_uni(kj, pos, A)) != 8 * want) fail("lane ^ (x | y)", a1, a2, a3, G::LT, pos, j0inv, tid, g * (1 << A) + p, lane ^ G::wr_uni(kj, pos, A), 8LL * want);
                        if ((x & ~(8 * (G::T - 1))) || (y & (8 * G::T - 1)) || (lane & y)) fail("fields overlap", a1, a2, a3, G::LT, pos, j0inv, tid, g * (1 << A) + p, x, y);
                    }
                    if (want < 0 || want >= G::R * G::T || seen[want]++) fail("not a permutation", a1, a2, a3, G::LT, pos, j0inv, tid, g * (1 << A) + p, want, want);
                    g_cases++;
                }
            }
        for (size_t i = 0; i < seen.size(); i++)
            if (seen[i] != 1) fail("tile not covered", a1, a2, a3, G::LT, pos, j0inv, -1, -1, (long long)i, seen[i]);
    }
}

template <int A1, int A2, int A3, int LOGT>
static void check_shape() {
    using G = Geo<A1, A2, A3, LOGT>;
    const long long before = g_cases;
    check_round<G>(A1, A2, A3, G::POS1, A1, false);
    if (G::J >= 3) check_round<G>(A1, A2, A3, G::POS2, A2, false);
    check_round<G>(A1, A2, A3, 0, G::AJ, true);
    // the transposing copy-out (the table form runs it on two-round shapes; the identity holds wherever a tile has 16 columns or more)
    bool copy_out = false;
    if constexpr (G::FACTORED && G::NT >= G::R) {
        copy_out = true;
        std::vector<unsigned char> seen((size_t)G::R * G::T);
        for (int tid = 0; tid < G::NT; tid++) {
            const int lane = G::rd_lane(tid);
            for (int i = 0; i < 16; i++) {
                const int idx = i * G::NT + tid;
                const int k = idx & (G::R - 1), t2 = idx >> G::L;
                const int want = G::lpos(G::sigma_of_k(k), t2);
                if ((lane ^ G::rd_xor(i)) != 8 * want) fail("copy-out read", A1, A2, A3, LOGT, -1, 0, tid, i, lane ^ G::rd_xor(i), 8LL * want);
                if (G::kof(G::sigma_of_k(k)) != k) fail("kof(sigma_of_k)", A1, A2, A3, LOGT, -1, 0, tid, i, G::kof(G::sigma_of_k(k)), k);
                if (want < 0 || want >= G::R * G::T || seen[want]++) fail("copy-out: not a permutation", A1, A2, A3, LOGT, -1, 0, tid, i, want, want);
                g_cases++;
            }
        }
    }
    std::printf("shape %d %d %d %d factored %d copy_out %d cases %lld\n", A1, A2, A3, LOGT, G::FACTORED ? 1 : 0, copy_out ? 1 : 0, g_cases - before);
}

int main() {
#define X(A1, A2, A3, LOGT) check_shape<A1, A2, A3, LOGT>();
    ZP_NTT_SHAPES(X)
#undef X
    std::printf("ok: %lld\n", g_cases);
    return 0;
}
