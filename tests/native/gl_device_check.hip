// Device check of the hand-written Goldilocks forms of eigen_zeth_amd/csrc/gl_asm.hpp and of the device lowering of gl.hpp (test
// infrastructure): one kernel per primitive, one element per lane, results compared on the host with unsigned __int128 arithmetic on
// the corner operands of field_corners.hpp.  Built by tests/test_field_corners.py once per scratch window (-DGL_ASM_SCRATCH_BASE=116 / 52).
// Exit status: 0 all equal and every class hit, 1 a mismatch or an empty class, 2 a HIP error.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gl_asm.hpp"
#include "field_corners.hpp"

#define CK(x)                                                                                   \
    do {                                                                                        \
        const hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            fflush(stdout);                                                                     \
            exit(2);                                                                            \
        }                                                                                       \
    } while (0)

using fc::ref_add;
using fc::ref_mul;
using fc::ref_sub;
typedef unsigned __int128 u128;

// ---- kernels: lane i takes element i; nothing is read or written at i >= n
#define LANE(n)                                              \
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;     \
    if (i >= (n)) return

template <bool WEAK>
__global__ void k_mul2(const u64 *a, const u64 *b, const u64 *c, const u64 *d, u64 *ra, u64 *rc, u32 n) {
    LANE(n);
    u64 x = a[i], y = c[i];
    if constexpr (WEAK) gl_mul2w(x, b[i], y, d[i]);
    else gl_mul2(x, b[i], y, d[i]);
    ra[i] = x;
    rc[i] = y;
}
enum { OP_MUL1, OP_MUL1W, OP_MUL, OP_ADD, OP_SUB };
template <int OP>
__global__ void k_bin(const u64 *a, const u64 *b, u64 *r, u32 n) {
    LANE(n);
    if constexpr (OP == OP_MUL1) r[i] = gl_mul1(a[i], b[i]);
    else if constexpr (OP == OP_MUL1W) r[i] = gl_mul1w(a[i], b[i]);
    else if constexpr (OP == OP_MUL) r[i] = gl_mul(a[i], b[i]);
    else if constexpr (OP == OP_ADD) r[i] = gl_add(a[i], b[i]);
    else r[i] = gl_sub(a[i], b[i]);
}
__global__ void k_bfly2(const u64 *xa, const u64 *ya, const u64 *xb, const u64 *yb, u64 *sa, u64 *da, u64 *sb, u64 *db, u32 n) {
    LANE(n);
    u64 p = xa[i], q = ya[i], r = xb[i], s = yb[i];
    gl_bfly2(p, q, r, s);
    sa[i] = p;
    da[i] = q;
    sb[i] = r;
    db[i] = s;
}
template <int E>
__global__ void k_shl(const u64 *x, u64 *r_asm, u64 *r_c, u32 n) {
    LANE(n);
    r_asm[i] = gl_shl12<E>(x[i]);
    r_c[i] = gl_mul_pow2<12 * E>(x[i]);
}
// the k-th product of lane i's sequence: operands walk the array with two strides
__host__ __device__ inline void seq_idx(u32 lane, u32 k, u32 nops, u32 &ia, u32 &ib) {
    ia = (lane * 131u + k * 7u) % nops;
    ib = (lane * 31u + k * 17u + 5u) % nops;
}
__global__ void k_acc_seq(const u64 *ops, u32 nops, u32 len, u64 *r, u32 n) {
    LANE(n);
    gl_acc s = gl_acc_zero();
    for (u32 k = 0; k < len; k++) {
        u32 ia, ib;
        seq_idx(i, k, nops, ia, ib);
        gl_acc_mac(s, ops[ia], ops[ib]);
    }
    r[i] = gl_acc_reduce(s);
}
// iters products per lane, a b0 and a b1 in turn: every wrap counter grows
__global__ void k_acc_wrap(const u64 *a, const u64 *b0, const u64 *b1, u32 iters, u64 *r, u32 n) {
    LANE(n);
    gl_acc s = gl_acc_zero();
    const u64 x = a[i], y0 = b0[i], y1 = b1[i];
    for (u32 k = 0; k < iters; k++) gl_acc_mac(s, x, (k & 1) ? y1 : y0);
    r[i] = gl_acc_reduce(s);
}
// gl_acc_reduce on a constructed state (the device struct: the host pass has another one)
__global__ void k_acc_state(const u64 *a, const u64 *b, const u64 *c, const u32 *oa, const u32 *ob, const u32 *oc, u64 *r, u32 n) {
#if defined(__HIP_DEVICE_COMPILE__)
    LANE(n);
    const gl_acc s = gl_acc{a[i], b[i], c[i], oa[i], ob[i], oc[i]};
    r[i] = gl_acc_reduce(s);
#endif
}

// ---- host side
template <class T>
struct dbuf {
    T *p;
    size_t n;
    explicit dbuf(size_t n_) : p(nullptr), n(n_) {
        CK(hipMalloc((void **)&p, n * sizeof(T)));
        CK(hipMemset(p, 0xA5, n * sizeof(T)));
    }
    explicit dbuf(const std::vector<T> &h) : p(nullptr), n(h.size()) {
        CK(hipMalloc((void **)&p, n * sizeof(T)));
        CK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    ~dbuf() { (void)hipFree(p); }
    std::vector<T> get() const {
        std::vector<T> h(n);
        CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
    dbuf(const dbuf &) = delete;
    dbuf &operator=(const dbuf &) = delete;
};
static inline dim3 grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
static void sync() {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}
static std::vector<u64> rotated(const std::vector<u64> &v, size_t by) {
    std::vector<u64> r(v.size());
    for (size_t i = 0; i < v.size(); i++) r[i] = v[(i + by) % v.size()];
    return r;
}

static u64 bad = 0;
static int empty = 0;
// a canonical-output primitive: equal bit for bit, and below p
static void check_canon(fc::tally &t, u64 got, u64 want, u64 a, u64 b, const char *cls) {
    t.check(got, want, a, b, cls);
    if (got >= fc::P) t.check(1, 0, a, got, "result not below p");
}

template <bool WEAK>
static void run_mul2(const char *name, const std::vector<u64> &A, const std::vector<u64> &B) {
    // stream P = every pair of E x E, stream Q = P rotated: (P, Q) in the slots (first, second), then (Q, P)
    const size_t n = A.size(), rot = 12347;
    const std::vector<u64> C = rotated(A, rot), D = rotated(B, rot);
    dbuf<u64> da(A), db(B), dc(C), dd(D), ra(n), rc(n);
    char n1[64], n2[64];
    snprintf(n1, sizeof n1, "%s.slot1", name);
    snprintf(n2, sizeof n2, "%s.slot2", name);
    fc::tally t1(n1), t2(n2);
    fc::class_table c1(n1), c2(n2);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0) k_mul2<WEAK><<<grid(n), 256>>>(da.p, db.p, dc.p, dd.p, ra.p, rc.p, (u32)n);
        else k_mul2<WEAK><<<grid(n), 256>>>(dc.p, dd.p, da.p, db.p, ra.p, rc.p, (u32)n);
        sync();
        const std::vector<u64> g1 = ra.get(), g2 = rc.get();
        const std::vector<u64> &a1 = pass ? C : A, &b1 = pass ? D : B, &a2 = pass ? A : C, &b2 = pass ? B : D;
        for (size_t i = 0; i < n; i++) {
            if (WEAK) {
                t1.check(g1[i] % fc::P, ref_mul(a1[i], b1[i]), a1[i], b1[i], fc::mul_class_name(a1[i], b1[i]));
                t2.check(g2[i] % fc::P, ref_mul(a2[i], b2[i]), a2[i], b2[i], fc::mul_class_name(a2[i], b2[i]));
            } else {
                check_canon(t1, g1[i], ref_mul(a1[i], b1[i]), a1[i], b1[i], fc::mul_class_name(a1[i], b1[i]));
                check_canon(t2, g2[i], ref_mul(a2[i], b2[i]), a2[i], b2[i], fc::mul_class_name(a2[i], b2[i]));
            }
            if (pass == 0) c1.hit_mul(a1[i], b1[i]);   // stream P in the first slot ...
            else c2.hit_mul(a2[i], b2[i]);             // ... and in the second
        }
    }
    bad += t1.print() + t2.print();
    empty += c1.print() + c2.print();
}

template <int OP>
static void run_bin(const char *name, const std::vector<u64> &A, const std::vector<u64> &B) {
    const size_t n = A.size();
    dbuf<u64> da(A), db(B), r(n);
    k_bin<OP><<<grid(n), 256>>>(da.p, db.p, r.p, (u32)n);
    sync();
    const std::vector<u64> g = r.get();
    fc::tally t(name);
    fc::class_table c(name);
    for (size_t i = 0; i < n; i++) {
        const u64 a = A[i], b = B[i];
        if (OP == OP_MUL1W) t.check(g[i] % fc::P, ref_mul(a, b), a, b, fc::mul_class_name(a, b));
        else if (OP == OP_MUL1 || OP == OP_MUL) check_canon(t, g[i], ref_mul(a, b), a, b, fc::mul_class_name(a, b));
        else if (OP == OP_ADD) check_canon(t, g[i], ref_add(a, b), a, b, fc::ADD_C[fc::add_class(a, b)]);
        else check_canon(t, g[i], ref_sub(a, b), a, b, fc::SUB_C[fc::sub_class(a, b)]);
        if (OP == OP_ADD) c.hit_add(a, b);
        else if (OP == OP_SUB) c.hit_sub(a, b);
        else c.hit_mul(a, b);
    }
    bad += t.print();
    empty += c.print();
}

static void run_bfly2(const std::vector<u64> &X, const std::vector<u64> &Y) {
    // every pair of E_c x E_c in slot a while slot b takes a rotated copy, then the other way round
    const size_t n = X.size(), rot = 4099;
    const std::vector<u64> XR = rotated(X, rot), YR = rotated(Y, rot);
    dbuf<u64> dx(X), dy(Y), dxr(XR), dyr(YR), sa(n), da(n), sb(n), db(n);
    fc::tally ta("gl_bfly2.slot_a"), tb("gl_bfly2.slot_b");
    fc::class_table ca("gl_bfly2.slot_a"), cb("gl_bfly2.slot_b");
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0) k_bfly2<<<grid(n), 256>>>(dx.p, dy.p, dxr.p, dyr.p, sa.p, da.p, sb.p, db.p, (u32)n);
        else k_bfly2<<<grid(n), 256>>>(dxr.p, dyr.p, dx.p, dy.p, sa.p, da.p, sb.p, db.p, (u32)n);
        sync();
        const std::vector<u64> gsa = sa.get(), gda = da.get(), gsb = sb.get(), gdb = db.get();
        const std::vector<u64> &xa = pass ? XR : X, &ya = pass ? YR : Y, &xb = pass ? X : XR, &yb = pass ? Y : YR;
        for (size_t i = 0; i < n; i++) {
            check_canon(ta, gsa[i], ref_add(xa[i], ya[i]), xa[i], ya[i], fc::ADD_C[fc::add_class(xa[i], ya[i])]);
            check_canon(ta, gda[i], ref_sub(xa[i], ya[i]), xa[i], ya[i], fc::SUB_C[fc::sub_class(xa[i], ya[i])]);
            check_canon(tb, gsb[i], ref_add(xb[i], yb[i]), xb[i], yb[i], fc::ADD_C[fc::add_class(xb[i], yb[i])]);
            check_canon(tb, gdb[i], ref_sub(xb[i], yb[i]), xb[i], yb[i], fc::SUB_C[fc::sub_class(xb[i], yb[i])]);
            if (pass == 0) { ca.hit_add(xa[i], ya[i]); ca.hit_sub(xa[i], ya[i]); }
            else { cb.hit_add(xb[i], yb[i]); cb.hit_sub(xb[i], yb[i]); }
        }
    }
    bad += ta.print() + tb.print();
    empty += ca.print() + cb.print();
}

template <int E>
static void run_shl(fc::tally &ta, fc::tally &tc, const std::vector<u64> &ec) {
    const std::vector<u64> X = fc::with_preimages(ec, 12 * E);
    const size_t n = X.size();
    dbuf<u64> dx(X), ra(n), rc(n);
    k_shl<E><<<grid(n), 256>>>(dx.p, ra.p, rc.p, (u32)n);
    sync();
    const std::vector<u64> ga = ra.get(), gc = rc.get();
    for (size_t i = 0; i < n; i++) {
        const u64 want = fc::ref_shl(X[i], 12 * E);
        check_canon(ta, ga[i], want, X[i], (u64)E, "gl_shl12<b>");
        check_canon(tc, gc[i], want, X[i], (u64)(12 * E), "gl_mul_pow2<b>");
    }
    if constexpr (E < 7) run_shl<E + 1>(ta, tc, ec);
}

static void run_acc(const std::vector<u64> &E) {
    fc::tally ts("gl_acc.sequences"), tw("gl_acc.wrap_counters"), tr("gl_acc_reduce.states");
    {   // sums of 1, 2, 3, 17 and 4096 products per lane
        const u32 LEN[5] = {1, 2, 3, 17, 4096}, lanes = 1024, nops = (u32)E.size();
        dbuf<u64> ops(E), r(lanes);
        for (int l = 0; l < 5; l++) {
            k_acc_seq<<<grid(lanes), 256>>>(ops.p, nops, LEN[l], r.p, lanes);
            sync();
            const std::vector<u64> g = r.get();
            for (u32 i = 0; i < lanes; i++) {
                u64 want = 0;
                for (u32 k = 0; k < LEN[l]; k++) {
                    u32 ia, ib;
                    seq_idx(i, k, nops, ia, ib);
                    want = ref_add(want, ref_mul(E[ia], E[ib]));
                }
                check_canon(ts, g[i], want, (u64)i, (u64)LEN[l], "lane, length");
            }
        }
    }
    {   // 2^20 products per lane of a maximal value with itself and with p - 1 in turn
        const u64 M[8] = {0xFFFFFFFEFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL, fc::P - 1, 0xFFFFFFFF80000000ULL, 0x80000000FFFFFFFFULL, 0xFFFFFFFFULL, fc::P, 1};
        std::vector<u64> a, b0, b1;
        for (int i = 0; i < 64; i++) {
            a.push_back(M[i & 7]);
            b0.push_back(i < 8 ? M[i & 7] : M[(i >> 3) & 7]);   // lanes 0..7: the value with itself
            b1.push_back(fc::P - 1);
        }
        const u32 iters = 1u << 20, n = 64;
        dbuf<u64> da(a), d0(b0), d1(b1), r(n);
        k_acc_wrap<<<grid(n), 256>>>(da.p, d0.p, d1.p, iters, r.p, n);
        sync();
        const std::vector<u64> g = r.get();
        for (u32 i = 0; i < n; i++) {
            const u64 want = ref_mul(iters / 2, ref_add(ref_mul(a[i], b0[i]), ref_mul(a[i], b1[i])));
            check_canon(tw, g[i], want, a[i], b0[i], "2^19 (a b + a (p-1))");
        }
    }
    {   // constructed states: a + 2^64 oa + 2^32 (b + 2^64 ob) + 2^64 (c + 2^64 oc) mod p
        const u64 V[5] = {0, 1, 0xFFFFFFFFULL, 1ULL << 63, 0xFFFFFFFFFFFFFFFFULL};
        const u32 O[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
        std::vector<u64> a, b, c;
        std::vector<u32> oa, ob, oc;
        for (int i = 0; i < 125 * 64; i++) {
            a.push_back(V[i % 5]);
            b.push_back(V[i / 5 % 5]);
            c.push_back(V[i / 25 % 5]);
            oa.push_back(O[i / 125 % 4]);
            ob.push_back(O[i / 500 % 4]);
            oc.push_back(O[i / 2000 % 4]);
        }
        const u32 n = (u32)a.size();
        dbuf<u64> da(a), db(b), dc(c), r(n);
        dbuf<u32> doa(oa), dob(ob), doc(oc);
        k_acc_state<<<grid(n), 256>>>(da.p, db.p, dc.p, doa.p, dob.p, doc.p, r.p, n);
        sync();
        const std::vector<u64> g = r.get();
        const u64 t32 = 1ULL << 32, t64 = fc::ref_mod((u128)1 << 64);
        for (u32 i = 0; i < n; i++) {
            const u64 va = fc::ref_mod((u128)a[i] + ((u128)oa[i] << 64)), vb = fc::ref_mod((u128)b[i] + ((u128)ob[i] << 64)),
                      vc = fc::ref_mod((u128)c[i] + ((u128)oc[i] << 64));
            const u64 want = ref_add(ref_add(va, ref_mul(vb, t32)), ref_mul(vc, t64));
            check_canon(tr, g[i], want, (u64)i, 0, "state index");
        }
    }
    bad += ts.print() + tw.print() + tr.print();
}

int main() {
    int ndev = 0;
    CK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    CK(hipSetDevice(0));
    const std::vector<u64> E = fc::operands(), Ec = fc::canonical(E);
    printf("window %d operands %zu canonical %zu\n", GL_ASM_SCRATCH_BASE, E.size(), Ec.size());
    std::vector<u64> A, B, XA, XB;   // E x E, E_c x E_c
    for (size_t i = 0; i < E.size(); i++)
        for (size_t j = 0; j < E.size(); j++) { A.push_back(E[i]); B.push_back(E[j]); }
    for (size_t i = 0; i < Ec.size(); i++)
        for (size_t j = 0; j < Ec.size(); j++) { XA.push_back(Ec[i]); XB.push_back(Ec[j]); }

    run_mul2<false>("gl_mul2", A, B);
    run_mul2<true>("gl_mul2w", A, B);
    run_bin<OP_MUL1>("gl_mul1", A, B);
    run_bin<OP_MUL1W>("gl_mul1w", A, B);
    run_bin<OP_MUL>("gl_mul", A, B);
    run_bin<OP_ADD>("gl_add", XA, XB);   // canonical in, canonical out: E_c x E_c
    run_bin<OP_SUB>("gl_sub", XA, XB);
    run_bfly2(XA, XB);
    {
        fc::tally ta("gl_shl12"), tc("gl_mul_pow2");
        run_shl<1>(ta, tc, Ec);
        bad += ta.print() + tc.print();
    }
    run_acc(E);
    printf("total mismatches %llu empty classes %d\n", bad, empty);
    return (bad != 0 || empty != 0) ? 1 : 0;
}
