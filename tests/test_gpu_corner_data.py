"""Corner-case field elements through the C-ABI (-m gpu): the kernels that inline the hand-written Goldilocks forms -- NTT / LDE (window 116),
Poseidon and the Merkle tree (the weak forms, window 52), the out-of-domain evaluation, the DEEP quotient, the FRI fold and the stage-2 columns
(the device gl_acc) -- on whole arrays drawn from the canonical corner operands E_c of tests/native/field_corners.hpp, against the oracle, bit for
bit.  tests/test_field_corners.py runs each primitive alone; here register pressure, scheduling and the code around them are the kernels' own.
Uniformly random data, which every other parity test uses, reaches two of the nine carry / borrow classes of a product."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
P = O.P
M64 = (1 << 64) - 1


def corner_operands():
    """E of tests/native/field_corners.hpp, the same values in the same order"""
    e = []
    for k in range(64):
        b = 1 << k
        e += [b, b - 1, b + 1, P - b, P - b - 1, P - b + 1, ~b & M64, -b & M64]
    return e + [0, P, P + 1, M64, 0xFFFFFFFEFFFFFFFF, 0x7FFFFFFF00000000]


E = corner_operands()
EC = np.array([v for v in E if v < P], dtype=np.uint64)
EC_NONZERO = EC[EC != 0]
assert len(E) == 518 and len(EC) == 450


def corners(shape, seed, nonzero=False):
    """seeded choice from E_c"""
    return np.ascontiguousarray(np.random.default_rng(seed).choice(EC_NONZERO if nonzero else EC, size=shape))


def ext_point(seed):
    """an extension-field point with every component a non-zero corner: outside the base field, so on no evaluation domain, and
    (c + g0, g1, g2) is non-zero whatever c is"""
    z = [int(v) for v in corners((3,), seed, nonzero=True)]
    assert z[1] != 0 and z[2] != 0
    return z


@pytest.fixture(scope="module")
def ntt_case():
    """per size: the columns and what the oracle makes of them, computed once"""
    cache = {}

    def get(logn):
        if logn not in cache:
            n = 1 << logn
            x = np.empty((5, n), dtype=np.uint64)
            x[:2] = corners((2, n), 0xC0 + logn)
            x[2] = P - 1
            x[3, 0::2], x[3, 1::2] = P - 1, 1
            x[4] = 0xFFFFFFFEFFFFFFFF
            x.setflags(write=False)
            cache[logn] = (x, O.ntt(x), O.intt(x), {logb: O.lde(x, logb) for logb in (0, 1, 2)})
        return cache[logn]
    return get


@pytest.mark.parametrize("logn,limb", [(4, 0), (8, 0), (12, 0), (13, 0), (16, 0), (13, 1), (16, 1)])
def test_ntt_intt_lde_on_corner_columns(prover, ntt_case, logn, limb):
    x, fwd, inv, ext = ntt_case(logn)
    W, n = x.shape
    d_in, d_out = prover.upload(x), prover.alloc(W * n)
    prover.set_tuning("ntt_limb", limb)
    try:
        prover.ntt(d_in, d_out, logn, W)
        assert (prover.download(d_out, x.shape) == fwd).all()
        prover.intt(d_in, d_out, logn, W)
        assert (prover.download(d_out, x.shape) == inv).all()
        prover.intt(prover.upload(fwd), d_out, logn, W)
        assert (prover.download(d_out, x.shape) == x).all()
        for logb in (0, 1, 2):          # blow-up 1, 2 and 4
            d_ext = prover.alloc(W << (logn + logb))
            prover.lde(d_in, d_ext, logn, logb, W)
            assert (prover.download(d_ext, ext[logb].shape) == ext[logb]).all(), logb
            d_ext.free()
    finally:
        prover.set_tuning("ntt_limb", 0)
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("count", [1, 5, 64, 65, 4096])
def test_poseidon_on_corner_states(prover, tables, count):
    """the latency kernel (<= 64 states) and the throughput kernel"""
    rc, mds = tables
    st = corners((count, 12), 0xA0 + count)
    st[0] = P - 1
    if count > 2:
        st[1] = 0xFFFFFFFEFFFFFFFF
        st[2] = 0
    d = prover.upload(st)
    prover.poseidon_perm(d, count)
    assert (prover.download(d, st.shape) == O.poseidon_perm(st, rc, mds)).all()


@pytest.mark.parametrize("M,W", [(64, 5), (64, 12), (1024, 5), (1024, 12)])
def test_merkle_on_corner_leaves(prover, tables, M, W):
    rc, mds = tables
    cols = corners((W, M), 0xB0 + W + M)
    cols[0, :3] = [P - 1, 0, 0xFFFFFFFEFFFFFFFF]
    cols[:, 3] = P - 1
    ref = O.merkle_commit(cols, rc, mds)
    d_tree = prover.alloc((2 * M - 1) * 4)
    prover.merkle_commit(prover.upload(cols), M, W, d_tree)
    assert (prover.download(d_tree, ref.shape) == ref).all()
    prover.merkle_commit_rows(prover.upload(np.ascontiguousarray(cols.T)), M, W, d_tree)
    assert (prover.download(d_tree, ref.shape) == ref).all()


@pytest.mark.parametrize("nblocks,extra", [(0, 1), (1, 0), (7, 2)])
def test_sponge_on_corner_blocks(prover, tables, nblocks, extra):
    rc, mds = tables
    state = [int(v) for v in corners((12,), 0xD0 + nblocks)]
    blocks = [[int(v) for v in corners((8,), 0xD1 + 16 * nblocks + i)] for i in range(nblocks)]
    perm = lambda st: [int(v) for v in O.poseidon_perm(np.array([st], dtype=np.uint64), rc, mds)[0]]
    st, rates = list(state), []
    if not blocks:
        st = perm(st)
    for b in blocks:
        st = perm(b + st[8:])
    rates.append(st[:8])
    for _ in range(extra):
        st = perm(st)
        rates.append(st[:8])
    got_state, got_rates = prover.poseidon_sponge(state, blocks, extra)
    assert got_state == st and got_rates == rates


@pytest.mark.parametrize("logn", [4, 9, 12])
def test_poly_eval_ext_on_corner_coefficients(prover, logn):
    W = 3
    coef = corners((W, 1 << logn), 0xE0 + logn)
    coef[2] = P - 1
    for z in (ext_point(0xE1 + logn), [P - 1, P - 1, P - 1], [0xFFFFFFFEFFFFFFFF, 0, 0]):
        got = prover.poly_eval_ext(prover.upload(coef), logn, W, z)
        assert (got == O.poly_eval_e3_cols(coef, z)).all(), z


@pytest.mark.parametrize("logn", [4, 9, 12])
@pytest.mark.parametrize("shift", [49, 1])
def test_ood_eval_on_corner_columns(prover, logn, shift):
    """as tests/test_gpu_stark.py lays it out: the values of the interpolants on shift <w_M> (blow-up 2), evaluated at z and z w from the
    sub-coset, against the coefficient form"""
    W, logb = 3, 1
    n, M = 1 << logn, 1 << (logn + logb)
    x = corners((W, n), 0xF0 + logn)
    x[2] = P - 1
    coef = O.intt(x)
    pad = np.zeros((W, M), dtype=np.uint64)
    pad[:, :n] = O.coset_scaled_coefficients(x, shift)
    d_ext = prover.upload(O.ntt(pad))
    wn = pow(O.ROOT32_DEFAULT, 1 << (32 - logn), P)
    base = 1 << 32                                   # a base-field corner: of order 6, so off every coset of a 2^k-th roots' group with this shift
    assert pow(base * pow(shift, -1, P) % P, n, P) != 1
    for z in (ext_point(0xF1 + logn), [P - 1, 1, 0xFFFFFFFEFFFFFFFF], [base, 0, 0]):
        zw = [v * wn % P for v in z]
        got_z, got_zw = prover.ood_eval(d_ext, M, 1 << logb, W, logn, shift, z, want_next=True)
        assert (got_z == O.poly_eval_e3_cols(coef, z)).all(), z
        assert (got_zw == O.poly_eval_e3_cols(coef, zw)).all(), z
    d_ext.free()


@pytest.mark.parametrize("logm,Wa,Wb,nn", [(6, 3, 0, 0), (10, 5, 3, 5), (12, 4, 3, 2)])
def test_deep_quotient_on_corner_columns(prover, logm, Wa, Wb, nn):
    a = corners((Wa, 1 << logm), 0x150)
    a[0] = P - 1
    b = corners((max(Wb, 1), 1 << logm), 0x151)
    z, zw, g = (ext_point(s) for s in (0x152, 0x153, 0x154))      # off the domain: the denominators x - z, x - z w are not zero
    ez = corners((Wa + Wb, 3), 0x155)
    ezw = corners((max(nn, 1), 3), 0x156)
    ez[0] = P - 1
    ref = O.deep_quotient(a, b[:Wb] if Wb else None, nn, z, zw, g, ez, ezw[:nn] if nn else None)
    d_out = prover.alloc(3 << logm)
    prover.deep_quotient(prover.upload(a), Wa, prover.upload(b) if Wb else None, Wb, logm, nn, z, zw, g, ez, ezw, 49, d_out)
    assert (prover.download(d_out, (3, 1 << logm)) == ref).all()


@pytest.mark.parametrize("logn", [4, 10, 14])
@pytest.mark.parametrize("logf", [1, 2, 3, 4])
def test_fri_fold_on_corner_data(prover, logn, logf):
    planes = corners((3, 1 << logn), 0x160 + logn)
    planes[:, :2] = P - 1
    for beta in (ext_point(0x161 + logf), [P - 1, P - 1, P - 1]):
        ref = O.fri_fold(planes, logf, beta, 49)
        d_out = prover.alloc(3 << (logn - logf))
        prover.fri_fold(prover.upload(planes), d_out, logn, logf, beta, 49)
        assert (prover.download(d_out, ref.shape) == ref).all(), beta


@pytest.mark.parametrize("n", [17, 4097])
def test_grand_product_on_corner_data(prover, n):
    a = corners((n,), 0x170 + n)
    b = a[np.random.default_rng(0x171).permutation(n)]
    for g in (ext_point(0x172), [0, P - 1, 0xFFFFFFFEFFFFFFFF]):
        assert g[1] != 0 or g[2] != 0                   # (b_i + g0, g1, g2) is never zero: every quotient exists
        d_out = prover.alloc(3 * n)
        prover.grand_product(prover.upload(a), prover.upload(b), n, g, d_out)
        assert (prover.download(d_out, (3, n)) == O.grand_product(a, b, g)).all(), g


@pytest.mark.parametrize("n", [17, 4097])
def test_logup_columns_on_corner_data(prover, n):
    a, t_, m = (corners((n,), 0x180 + n + i) for i in range(3))      # the kernel does not care whether the lookup holds
    for g in (ext_point(0x183), [0, P - 1, 0xFFFFFFFEFFFFFFFF]):
        assert g[1] != 0 or g[2] != 0                   # (a_i + g0, g1, g2) and (t_i + g0, g1, g2) are never zero
        d_out = prover.alloc(9 * n)
        prover.logup_columns(prover.upload(a), prover.upload(t_), prover.upload(m), n, g, d_out)
        assert (prover.download(d_out, (9, n)) == O.logup_columns(a, t_, m, g)).all(), g
