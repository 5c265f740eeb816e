// Tile geometry of the NTT pass kernels (ntt.hip): which LDS position a slot of the radix-R tile takes, and the factored
// form of that position the kernels compute.  Plain C++ as well as device code: tests/native/ntt_slots_check.cpp walks
// every shape, round, root class, lane and register on the host.
#pragma once

#if defined(__HIPCC__)
#define GEO_HD __host__ __device__ __forceinline__
#else
#define GEO_HD inline
#endif

GEO_HD constexpr int brev(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}
// the slot of a round whose radix-2^A field sits at bit `pos`: o counts the other bits, j is the field
GEO_HD constexpr int slot_of(int o, int j, int pos, int A) {
    return ((o >> pos) << (pos + A)) | (j << pos) | (o & ((1 << pos) - 1));
}

template <int A1, int A2, int A3, int LOGT>
struct Geo {
    static constexpr int L = A1 + A2 + A3;
    static constexpr int R = 1 << L;
    static constexpr int T = 1 << LOGT;
    static constexpr int LT = LOGT;
    static constexpr int NT = (R * T) / 16;
    static constexpr int J = 1 + (A2 > 0 ? 1 : 0) + (A3 > 0 ? 1 : 0);
    static constexpr int POS1 = L - A1;
    static constexpr int POS2 = L - A1 - A2;
    static constexpr int AJ = (J == 1) ? A1 : (J == 2 ? A2 : A3);
    // output index k held by slot sigma once all rounds are done
    GEO_HD static constexpr int kof(int sigma) {
        int k = (sigma >> POS1) & ((1 << A1) - 1);
        if (A2 > 0) k |= ((sigma >> POS2) & ((1 << A2) - 1)) << A1;
        if (A3 > 0) k |= (sigma & ((1 << A3) - 1)) << (A1 + A2);
        return k;
    }
    GEO_HD static constexpr int sigma_of_k(int k) {
        int s = (k & ((1 << A1) - 1)) << POS1;
        if (A2 > 0) s |= ((k >> A1) & ((1 << A2) - 1)) << POS2;
        if (A3 > 0) s |= (k >> (A1 + A2)) & ((1 << A3) - 1);
        return s;
    }
    // LDS position of (slot sigma, column t).  t is XORed with the low bits of the output index (conflict-free row accesses
    // and transposing copy-out at T >= 16).  With T < 16 one slot is only T*8 < 128 bytes, so the 32 lanes of a half-wave
    // span 32/T slots and those must fall into different 32/T-ths of a 256-byte bank row: the low bits of sigma (inside
    // the last-round field) are XORed with the low bits of the middle field (last-round reads and writes: consecutive lanes
    // = consecutive middle-field values) and, one bit up, with the top-field bits the t-swizzle does not use (transposing
    // copy-out: consecutive lanes = consecutive top-field values, then the middle field steps by one).
    GEO_HD static constexpr int lpos(int sigma, int t) {
        int s2 = sigma;
        if constexpr (LOGT < 4 && A3 > 0) {
            constexpr int GB = 5 - LOGT;
            s2 ^= ((sigma >> POS2) & ((1 << GB) - 1)) ^ (((sigma >> (POS1 + LOGT)) & ((1 << (A1 - LOGT)) - 1)) << 1);
        }
        return (s2 << LOGT) + (t ^ (kof(sigma) & (T - 1)));
    }

    // ---- lpos in factors.  Without the slot swizzle above (every shape with T >= 16 or two rounds: all but the radix-2^11 and
    // 2^12 tiles of 8, 4 and 2 columns, which keep lpos) the position is made of bit fields only: slot_of puts o and the field j into
    // disjoint bits, kof moves bits around, so both split over (o, t) and j, and as a BYTE offset
    //     8 lpos(slot_of(o, j, pos, A), t)  =  (wr_lane(o, t, pos, A) ^ wr_xor(j, pos, A)) + wr_add(j, pos, A)
    // wr_lane is per lane and the same for every register of a round: made once per round.  wr_xor (inside the t field: the part
    // of the swizzle that takes j -- the round's own field of a first exchange; zero where the field lies above T's bits of k) and
    // wr_add (above it: the slot bits of j) are wave-uniform with j = k_j: scalar work.  The three occupy disjoint bits, so the sum
    // is also  wr_lane ^ wr_uni  with one uniform operand, wr_uni = wr_xor | wr_add: gfx950 reads one scalar register per VALU
    // instruction, and this is the form that is one instruction per write.
    static constexpr bool FACTORED = !(LOGT < 4 && A3 > 0);
    GEO_HD static constexpr int wr_lane(int o, int t, int pos, int A) { return lpos(slot_of(o, 0, pos, A), t) << 3; }
    GEO_HD static constexpr int wr_xor(int j, int pos, int A) { return (kof(slot_of(0, j, pos, A)) & (T - 1)) << 3; }
    GEO_HD static constexpr int wr_add(int j, int pos, int A) { return slot_of(0, j, pos, A) << (LOGT + 3); }
    GEO_HD static constexpr int wr_uni(int j, int pos, int A) { return wr_xor(j, pos, A) | wr_add(j, pos, A); }
    GEO_HD static constexpr int wr_pos(int lane, int x, int y) { return (lane ^ x) + y; }
    // The transposing copy-out reads element idx = i NT + tid of the tile in output order, k = idx mod R, column t2 = idx / R.  NT is
    // R T / 16, so k = tid mod R whatever i is and t2 = i T/16 + tid / R: the byte offset of lpos(sigma_of_k(k), t2) is the lane's
    // rd_lane XOR the constant rd_xor(i)  (T = 16: k = tid, t2 = i)
    GEO_HD static constexpr int rd_lane(int tid) { return lpos(sigma_of_k(NT == R ? tid : (tid & (R - 1))), NT == R ? 0 : (tid >> L)) << 3; }
    GEO_HD static constexpr int rd_xor(int i) { return (i * (NT >> L)) << 3; }
};

// the shapes dispatch_pass builds: A1, A2, A3, LOGT (the 64-bit-offset forms share their geometry)
#define ZP_NTT_SHAPES(X) \
    X(3, 2, 0, 5) X(3, 3, 0, 5) X(4, 3, 0, 5) X(4, 4, 0, 4) X(4, 4, 0, 5) X(3, 3, 3, 4) X(3, 3, 3, 5) X(4, 3, 3, 4) X(4, 4, 3, 3) X(4, 4, 4, 1) X(4, 4, 4, 2)
