"""GPU tests of the STARK stage (-m gpu): per-kernel parity against the oracle, then whole proofs:
the MI355X proof must (a) be bit-identical to the proof the CPU restatement produces from the same
witness and (b) pass the independent verifier (oracle/stark_verify.py)."""
import copy
import os
import re

import numpy as np
import pytest

import witness_cases as WC
from test_witness_check_host import host_check, raw_check
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR
from oracle import naive as NV
from oracle import oracle as O
from oracle import stark_verify as V
from oracle.stark_cpu import CpuBackend

pytestmark = pytest.mark.gpu
P = O.P


@pytest.fixture(scope="module")
def hip_backend(prover):
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    return HipBackend(prover=prover)


@pytest.fixture(scope="module")
def cpu_backend(tables):
    return CpuBackend(*tables)


@pytest.mark.parametrize("logn,W", [(4, 1), (12, 3), (13, 5), (16, 2)])
def test_poly_eval_ext_matches_oracle(prover, logn, W):
    coef = O.random_field((W, 1 << logn), 40 + logn)
    z = O.random_field((3,), 41).tolist()
    got = prover.poly_eval_ext(prover.upload(coef), logn, W, z)
    assert (got == O.poly_eval_e3_cols(coef, z)).all()
    # base-field point embedded: must equal plain Horner
    got = prover.poly_eval_ext(prover.upload(coef), logn, W, [7, 0, 0])
    for c in range(W):
        assert got[c].tolist() == [O.poly_eval(coef[c], 7), 0, 0]


@pytest.mark.parametrize("logn,logb,W", [(0, 0, 1), (1, 1, 2), (4, 1, 1), (9, 0, 9), (12, 1, 3), (13, 2, 5), (16, 1, 6), (20, 1, 2)])
def test_ood_eval_from_values_matches_the_coefficient_definition(prover, logn, logb, W):
    """zp_ood_eval (barycentric form over the resident extension, round 5) against the oracle's definition: interpolate, then evaluate the
    coefficient form -- at zeta and at zeta w, from the 2^logn-point sub-coset of an extension with blow-up 2^logb (row stride 2^logb),
    on the coset (shift 49) and on the trace domain itself (shift 1), for a full ext point and a base-field point"""
    n, M = 1 << logn, 1 << (logn + logb)
    x = O.random_field((W, n), 0x00D0 + logn)
    coef = O.intt(x)                                                   # p_c(w^i) = x[c][i]
    wn = pow(O.ROOT32_DEFAULT, 1 << (32 - logn), P) if logn else 1
    for shift in (49, 1):
        # the columns as an extension would hold them: values of p on shift <w_M>, so that rows 0, 2^logb, ... are p(shift w_n^i)
        sc = np.array([[int(c) * pow(shift, i, P) % P for i, c in enumerate(row)] for row in coef.tolist()], dtype=np.uint64) if logn <= 13 else None
        if sc is None:      # large sizes: the library's own LDE lays the extension down (it is compared with the oracle elsewhere)
            if shift == 1:
                continue
            d_ext = prover.alloc(W * M)
            prover.lde(prover.upload(x), d_ext, logn, logb, W, shift)
        else:
            pad = np.zeros((W, M), dtype=np.uint64)
            pad[:, :n] = sc
            d_ext = prover.upload(O.ntt(pad))
        for z in (O.random_field((3,), 0x00D1 + logn).tolist(), [12345, 0, 0]):
            zw = [v * wn % P for v in z]
            got_z, got_zw = prover.ood_eval(d_ext, M, 1 << logb, W, logn, shift, z, want_next=True)
            assert (got_z == O.poly_eval_e3_cols(coef, z)).all()
            assert (got_zw == O.poly_eval_e3_cols(coef, zw)).all()
            assert (prover.ood_eval(d_ext, M, 1 << logb, W, logn, shift, z) == got_z).all()
        d_ext.free()
    # a point ON the domain is refused (the protocol excludes it), not answered with garbage
    if logn >= 1:
        d = prover.upload(x)
        with pytest.raises(native.ZpError):
            prover.ood_eval(d, n, 1, W, logn, 1, [pow(wn, 3, P), 0, 0])
        d.free()


@pytest.mark.parametrize("logm,Wa,Wb,nn", [(6, 3, 0, 0), (10, 5, 3, 5), (12, 4, 3, 2), (0, 1, 0, 0), (1, 1, 0, 1), (6, 3, 0, 3), (7, 1, 2, 1)])
def test_deep_quotient_matches_oracle(prover, logm, Wa, Wb, nn):
    a = O.random_field((Wa, 1 << logm), 50)
    b = O.random_field((max(Wb, 1), 1 << logm), 51)
    z, zw, g = (O.random_field((3,), s).tolist() for s in (52, 53, 54))
    ez = O.random_field((Wa + Wb, 3), 55)
    ezw = O.random_field((max(nn, 1), 3), 56)
    ref = O.deep_quotient(a, b[:Wb] if Wb else None, nn, z, zw, g, ez, ezw[:nn] if nn else None)
    assert (O.deep_quotient(a, b[:Wb] if Wb else None, nn, z, zw, g, ez, ezw[:nn] if nn else None, fast=True) == ref).all()
    d_out = prover.alloc(3 << logm)
    prover.deep_quotient(prover.upload(a), Wa, prover.upload(b) if Wb else None, Wb, logm, nn, z, zw, g, ez, ezw, 49, d_out)
    assert (prover.download(d_out, (3, 1 << logm)) == ref).all()


@pytest.mark.parametrize("nrows,Wa,Wb,nn,stride,base", [(1, 1, 0, 1, 1, 0), (255, 3, 2, 2, 256, 0), (257, 3, 2, 3, 258, 0), (257, 3, 0, 3, 259, 0), (257, 3, 2, 1, 258, 1)])
def test_deep_quotient_rows_odd_windows_strides_and_bases(prover, nrows, Wa, Wb, nn, stride, base):
    """zp_deep_quotient_rows against orc_deep_quotient_rows: windows of 1, 255 and 257 rows (a lane holds two rows: an odd count ends on
    half a lane), on even strides and 16-byte-aligned bases (each lane loads its row pair at once), on the odd column stride 259 and on a
    column base moved by one word (both turn the pair loads off)"""
    logm, row0 = 10, 301
    a = O.random_field((Wa, stride), 930 + nrows)
    b = O.random_field((max(Wb, 1), stride), 931 + nrows)
    z, zw, g = (O.random_field((3,), 932 + i).tolist() for i in range(3))
    ez, ezw = O.random_field((Wa + Wb, 3), 935), O.random_field((max(nn, 1), 3), 936)
    so = nrows + 1
    ref = np.zeros((3, so), dtype=np.uint64)
    O.lib().orc_deep_quotient_rows(O._p(a), Wa, stride, O._p(b), Wb, stride, logm, row0, nrows, nn, O._p(O._arr(z)), O._p(O._arr(zw)), O._p(O._arr(g)),
                                   O._p(ez), O._p(ezw), 49, O.ROOT32_DEFAULT, O._p(ref), so)
    pad = np.zeros(base, dtype=np.uint64)
    d_a, d_b = prover.upload(np.concatenate([pad, a.reshape(-1)])), prover.upload(np.concatenate([pad, b.reshape(-1)]))
    d_o = prover.alloc(3 * so)
    prover.memset(d_o, 0, 3 * so * 8)
    prover.deep_quotient_rows(d_a.offset(base), Wa, stride, d_b.offset(base) if Wb else None, Wb, stride, logm, row0, nrows, nn, z, zw, g, ez, ezw, 49, d_o, so)
    assert (prover.download(d_o, (3, so)) == ref).all()      # the word behind each plane's window stays 0


@pytest.mark.parametrize("r", [36, 37])
def test_deep_quotient_row_whose_denominator_vanishes(prover, r):
    """z = the domain's own point of row r (a protocol excludes it): include/zeth_prover.h says what the call leaves there -- row r is 0 in
    all three planes, where the checker keeps the term over x - zw -- and every other row, its lane partner r ^ 1 included, is exact"""
    logm, Wa, Wb, nn = 7, 1, 2, 1
    M = 1 << logm
    a, b = O.random_field((Wa, M), 940), O.random_field((Wb, M), 941)
    z = [49 * pow(NV.root(logm), r, P) % P, 0, 0]
    zw, g = (O.random_field((3,), 942 + i).tolist() for i in range(2))
    ez, ezw = O.random_field((Wa + Wb, 3), 944), O.random_field((nn, 3), 945)
    ref = O.deep_quotient(a, b, nn, z, zw, g, ez, ezw)
    d_out = prover.alloc(3 * M)
    prover.deep_quotient(prover.upload(a), Wa, prover.upload(b), Wb, logm, nn, z, zw, g, ez, ezw, 49, d_out)
    got = prover.download(d_out, (3, M))
    others = np.arange(M) != r
    assert (got[:, others] == ref[:, others]).all()
    assert got[:, r].tolist() == [0, 0, 0] and ref[:, r].tolist() != [0, 0, 0]


def test_stage2_columns_with_a_zero_denominator_match_the_checker(prover):
    """a base-field challenge g = (g0, 0, 0) that meets b[i] = -g0 (grand product) or a[i] = -g0 (LogUp) at i = 4096 + 5, in the second of
    three blocks: both sides read 1/0 as 0, so Z is 0 from row i + 1 on and h1[i] = 0; word for word against the checker"""
    n, i, g = 2 * 4096 + 17, 4096 + 5, [0x1234567, 0, 0]
    a = O.random_field((n,), 950)
    b = O.random_field((n,), 951)
    t_, m = O.random_field((n,), 952), np.random.default_rng(953).integers(0, 5, size=n, dtype=np.uint64)
    b[i] = P - g[0]
    assert (P - g[0]) not in a.tolist() + t_.tolist() and b.tolist().count(P - g[0]) == 1      # the one zero denominator is the planted one
    d_out = prover.alloc(3 * n)
    prover.grand_product(prover.upload(a), prover.upload(b), n, g, d_out)
    got = prover.download(d_out, (3, n))
    assert (got == O.grand_product(a, b, g)).all()
    assert not got[:, i + 1:].any() and got[:, i].any()
    a[i] = P - g[0]
    d_out = prover.alloc(9 * n)
    prover.logup_columns(prover.upload(a), prover.upload(t_), prover.upload(m), n, g, d_out)
    got = prover.download(d_out, (9, n))
    assert (got == O.logup_columns(a, t_, m, g)).all()
    assert got[0:3, i].tolist() == [0, 0, 0]


def test_gather_and_batch_open(prover, tables):
    rc, mds = tables
    M, W = 1 << 10, 7
    cols = O.random_field((W, M), 60)
    d = prover.upload(cols)
    idx = [0, M - 1, 5, 5, 777]
    assert (prover.gather_rows(d, M, W, idx) == cols[:, idx].T).all()
    tree = O.merkle_commit(cols, rc, mds)
    d_tree = prover.alloc((2 * M - 1) * 4)
    prover.merkle_commit(d, M, W, d_tree)
    paths = prover.merkle_open_batch(d_tree, M, idx)
    for i, j in enumerate(idx):
        assert (paths[i] == O.merkle_path(tree, j)).all()
    with pytest.raises(native.ZpError):
        prover.gather_rows(d, M, W, [M])


def _small_copy_words():
    """ZP_SMALL_COPY of csrc/ctx.hpp, in words: a query round trip of more (indices + outputs) leaves the staging route"""
    text = open(os.path.join(os.path.dirname(native.__file__), "csrc", "ctx.hpp")).read()
    a, b = re.search(r"#define ZP_SMALL_COPY \((\d+)u << (\d+)\)", text).groups()
    return (int(a) << int(b)) // 8


@pytest.fixture(scope="module")
def opened(prover, tables):
    """one set of columns at M = 2^10 with its binary tree (and the checker's) and a 16-ary BN254 tree, shared by the round-trip cases"""
    M, W = 1 << 10, 127
    cols = O.random_field((W, M), 61)
    d = prover.upload(cols)
    d_tree = prover.alloc((2 * M - 1) * 4)
    prover.merkle_commit(d, M, W, d_tree)
    prover.install_poseidon_bn254(17)
    d_tree16 = prover.alloc(prover.merkle16_nodes(M) * 4)
    prover.merkle16_commit_bn254(d, M, 3, d_tree16)
    return M, W, cols, d, d_tree, O.merkle_commit(cols, *tables), d_tree16


def test_query_round_trips_with_no_query_leave_the_outputs_alone(prover, opened):
    M, W, _, d, d_tree, _, d_tree16 = opened
    idx, out = np.zeros(1, dtype=np.uint64), np.full(64, 0xA5A5A5A5, dtype=np.uint64)
    lib, p = prover.lib, lambda a: a.ctypes.data_as(native._u64p)
    assert lib.zp_gather_rows(prover.ctx, d.ptr, M, W, p(idx), 0, p(out)) == 0
    assert lib.zp_merkle_open_batch(prover.ctx, d_tree.ptr, M, p(idx), 0, p(out)) == 0
    assert lib.zp_merkle16_open_batch_bn254(prover.ctx, d_tree16.ptr, M, idx.ctypes.data, 0, out.ctypes.data) == 0
    assert (out == 0xA5A5A5A5).all()


def test_query_round_trips_just_above_the_staging_threshold(prover, opened):
    """the smallest query counts whose indices and outputs together exceed ZP_SMALL_COPY: the Goldilocks pair leaves the staging buffer for
    scratch 3 there (the BN128 form always goes that way); every entry point against the same reference as below the threshold"""
    M, W, cols, d, d_tree, tree, d_tree16 = opened
    limit = _small_copy_words()
    rng = np.random.default_rng(62)
    draw = lambda per_query: rng.integers(0, M, size=limit // (per_query + 1) + 1, dtype=np.uint64)
    idx = draw(W)
    assert (len(idx) - 1) * (W + 1) <= limit < len(idx) * (W + 1)
    assert (prover.gather_rows(d, M, W, idx) == cols[:, idx.astype(np.int64)].T).all()
    idx = draw(10 * 4)
    assert (len(idx) - 1) * 41 <= limit < len(idx) * 41
    want = np.array([O.merkle_path(tree, j) for j in range(M)], dtype=np.uint64)
    assert (prover.merkle_open_batch(d_tree, M, idx) == want[idx.astype(np.int64)]).all()
    idx = draw(3 * 64)
    assert (len(idx) - 1) * 193 <= limit < len(idx) * 193
    paths = np.zeros((len(idx), 3, 16, 4), dtype=np.uint64)
    prover._chk(prover.lib.zp_merkle16_open_batch_bn254(prover.ctx, d_tree16.ptr, M, idx.ctypes.data, len(idx), paths.ctypes.data))
    single = np.zeros((M, 3, 16, 4), dtype=np.uint64)
    for j in sorted(set(idx.tolist())):
        prover._chk(prover.lib.zp_merkle16_open_bn254(prover.ctx, d_tree16.ptr, M, j, single[j].ctypes.data))
    assert (paths == single[idx.astype(np.int64)]).all()


def lookup_then_perm_air():
    """the range check and the permutation of the chunk AIR on its own trace (16 columns), the stage-2 table in the order LogUp, grand product:
    Z lives behind the nine LogUp planes, so a reader that advances by the wrong width after the first argument breaks every Z constraint"""
    width, Ww = 16, 8
    r, q, t, m = [AIR.Col(Ww + i) for i in (2, 3, 4, 5)]
    g = [AIR.Chal(i) for i in range(3)]
    s2 = lambda j, nxt=False: [AIR.Col(width + 3 * j + i, nxt) for i in range(3)]
    H1, H2, S, Sn, Z, Zn = s2(0), s2(1), s2(2), s2(2, True), s2(3), s2(3, True)
    ext = lambda v: [v + g[0], g[1], g[2]]
    p1, p2 = AIR.e3x_mul(H1, ext(r)), AIR.e3x_mul(H2, ext(t))
    lhs, rhs = AIR.e3x_mul(Zn, ext(q)), AIR.e3x_mul(Z, ext(r))
    cs = [p1[0] - 1, p1[1], p1[2], p2[0] - m, p2[1], p2[2]]
    cs += [Sn[i] - S[i] - H1[i] + H2[i] for i in range(3)] + [AIR.L_FIRST * S[i] for i in range(3)]
    cs += [lhs[i] - rhs[i] for i in range(3)] + [AIR.L_FIRST * (Z[0] - 1), AIR.L_FIRST * Z[1], AIR.L_FIRST * Z[2]]
    return AIR.Air("lookup_perm", width, 8, cs, trace_kind=3,
                   stage2=[{"kind": "lookup", "a": Ww + 2, "t": Ww + 4, "m": Ww + 5}, {"kind": "perm", "a": Ww + 2, "b": Ww + 3}])


def test_witness_check_of_a_logup_argument_followed_by_a_grand_product(prover):
    """both argument kinds in one stage-2 table, the nine-plane one first, at logn = 5: the verdict, the counts and the first rows of
    zp_stark_check_witness on the device equal the host checker's and the oracle's, on the satisfied trace and with the permutation broken"""
    logn = 5
    air = lookup_then_perm_air()
    blob = np.ascontiguousarray(air.program(), dtype=np.uint64)
    assert [int(blob[12 + int(blob[6]) + int(blob[7]) + 4 * k]) for k in range(2)] == [2, 1]      # the table's kinds: LogUp, grand product
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 11)
    pubs = [int(v) for v in pub]
    broken = WC.flipped(tr, 8 + 3, 7)            # q is no permutation of r any more: the grand product does not close
    for trace, verdict in ((tr, WC.SATISFIED), (broken, WC.VIOLATED)):
        for chal in (None, WC.EXPLICIT_CHALLENGE):
            want = WC.oracle_report(blob, trace, pubs, logn, chal)
            assert want[0][0] == verdict
            assert host_check(blob, trace, pubs, logn, chal) == want
            d = prover.upload(np.ascontiguousarray(trace, dtype=np.uint64))
            rc, rep, counts, first = raw_check(prover.ctx, blob, d.ptr, trace.size, pubs, logn, chal)
            d.free()
            assert rc == 0 and (rep, counts, first) == want


# rows the large stage-2 cases sample: the first blocks, the middle, the end, and both sides of block 256 -- where the scan of the block
# totals starts its second chunk with a carry (n = 2^20 + 4097 is 258 blocks of 4096; 2^20 is exactly one chunk of 256)
STAGE2_ROWS = [0, 1, 4095, 4096, (1 << 20) - 1, 1 << 20, (1 << 20) + 4095, (1 << 20) + 4096]


@pytest.mark.parametrize("n", [1, 2, 17, 4096, 4097, (1 << 16) + 5, 1 << 20, (1 << 20) + 4097])
def test_grand_product_matches_oracle(prover, n):
    a = O.random_field((n,), 80)
    b = a[np.random.default_rng(81).permutation(n)]
    g = O.random_field((3,), 82).tolist()
    d_out = prover.alloc(3 * n)
    prover.grand_product(prover.upload(a), prover.upload(b), n, g, d_out)
    got = prover.download(d_out, (3, n))
    if n <= (1 << 16) + 5:
        assert (got == O.grand_product(a, b, g)).all()
    else:   # size-independent properties: Z[0] = 1 and the recurrence at sampled rows
        assert got[:, 0].tolist() == [1, 0, 0]
        for i in [i for i in STAGE2_ROWS if i < n - 2] + [n // 2, n - 2]:
            zi = [int(got[c, i]) for c in range(3)]
            zn = [int(got[c, i + 1]) for c in range(3)]
            lhs = NV.e3_mul(zn, [(int(b[i]) + g[0]) % P, g[1], g[2]])
            assert lhs == NV.e3_mul(zi, [(int(a[i]) + g[0]) % P, g[1], g[2]])


@pytest.mark.parametrize("n", [1, 2, 17, 4096, 4097, (1 << 16) + 5, 1 << 20, (1 << 20) + 4097])
def test_logup_columns_match_oracle(prover, n):
    rng = np.random.default_rng(90)
    k = max(1, min(12, n.bit_length() - 1))
    a = rng.integers(0, 1 << k, size=n, dtype=np.uint64)
    t_ = (np.arange(n, dtype=np.uint64) % np.uint64(1 << k))
    m = rng.integers(0, 5, size=n, dtype=np.uint64)     # the kernel does not care whether the lookup holds
    g = O.random_field((3,), 91).tolist()
    d_out = prover.alloc(9 * n)
    prover.logup_columns(prover.upload(a), prover.upload(t_), prover.upload(m), n, g, d_out)
    got = prover.download(d_out, (9, n))
    if n <= (1 << 16) + 5:
        assert (got == O.logup_columns(a, t_, m, g)).all()
    else:   # definitions at sampled rows: h1 (a+g) = 1, h2 (t+g) = m, S' = S + h1 - h2, S[0] = 0
        assert got[6:9, 0].tolist() == [0, 0, 0]
        for i in [i for i in STAGE2_ROWS if i < n - 2] + [n // 2, n - 2]:
            h1 = [int(got[c, i]) for c in range(3)]
            h2 = [int(got[3 + c, i]) for c in range(3)]
            assert NV.e3_mul(h1, [(int(a[i]) + g[0]) % P, g[1], g[2]]) == [1, 0, 0]
            assert NV.e3_mul(h2, [(int(t_[i]) + g[0]) % P, g[1], g[2]]) == [int(m[i]), 0, 0]
            for c in range(3):
                assert int(got[6 + c, i + 1]) == (int(got[6 + c, i]) + h1[c] - h2[c]) % P


@pytest.mark.parametrize("name,logn", [("fib", 5), ("wide8", 8), ("wide32", 10)])
def test_constraint_kernel_matches_the_checkers_interpreter(hip_backend, cpu_backend, name, logn):
    """generated gfx950 kernel (product code generator) vs the checker's own interpreter of the constraint program blob
    (oracle/gl_oracle.c: orc_quotient_program) -- two lowerings that share no code"""
    air = AIR.get_air(name)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 99)
    from eigen_zeth_amd.stark import field as F
    apow = [O.random_field((3,), 70 + k).tolist() for k in range(len(air.constraints))]
    zhinv = [3, 5]
    wl = F.inv(F.root(logn, hip_backend.root32))
    q_cpu = cpu_backend.quotient(air, cpu_backend.commit_trace(tr, logn, 1), cpu_backend.fixed_ext(logn, 1), pub, apow, zhinv, logn, 1, wl)
    c1 = hip_backend.commit_trace(tr, logn, 1)
    d_q = hip_backend.quotient(air, c1, hip_backend.fixed_ext(logn, 1), pub, apow, zhinv, logn, 1, wl)
    assert (hip_backend.download(d_q, q_cpu.shape) == q_cpu).all()


@pytest.mark.parametrize("name,logn,queries", [("fib", 6, 5), ("fib", 12, 8), ("perm", 7, 6), ("perm", 13, 8), ("wide8", 10, 8), ("wide32", 13, 12), ("wide64", 14, 8), ("chunk16", 8, 6), ("chunk64", 13, 8)])
def test_gpu_proof_is_bit_identical_to_cpu_and_verifies(hip_backend, cpu_backend, tables, name, logn, queries):
    rc, mds = tables
    air = AIR.get_air(name)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 2024 + logn)
    params = PR.StarkParams(logn, logb=1, fri_logf=3, fri_final_log=4, n_queries=queries)
    gpu = PR.prove(air, tr, pub, params, hip_backend)
    cpu = PR.prove(air, tr, pub, params, cpu_backend)
    assert PR.proof_to_json(gpu) == PR.proof_to_json(cpu)
    assert V.verify(gpu, air.program(), rc, mds, V.expectation(params.to_dict()))
    bad = copy.deepcopy(gpu)
    bad["queries"][1]["fri"][0]["values"][0] ^= 1
    with pytest.raises(V.Reject):
        V.verify(bad, air.program(), rc, mds, V.expectation(params.to_dict()))


def test_gpu_rejects_bad_witness_downstream(hip_backend, tables):
    rc, mds = tables
    air = AIR.get_air("wide8")
    tr, pub = native.synth_trace(1, 9, 8, 3)
    tr[3, 100] = (int(tr[3, 100]) + 1) % P
    params = PR.StarkParams(9, 1, 3, 4, 6)
    proof = PR.prove(air, tr, pub, params, hip_backend)
    with pytest.raises(V.Reject):
        V.verify(proof, air.program(), rc, mds, V.expectation(params.to_dict()))


def test_blowup_four(hip_backend, cpu_backend, tables):
    rc, mds = tables
    air = AIR.get_air("fib")
    tr, pub = native.synth_trace(0, 9, 2, 8)
    params = PR.StarkParams(9, logb=2, fri_logf=2, fri_final_log=3, n_queries=6)
    gpu = PR.prove(air, tr, pub, params, hip_backend)
    assert PR.proof_to_json(gpu) == PR.proof_to_json(PR.prove(air, tr, pub, params, cpu_backend))
    assert V.verify(gpu, air.program(), rc, mds, V.expectation(params.to_dict()))


@pytest.mark.parametrize("name,logn", [("wide64", 22), ("wide8", 24), ("perm", 22), ("chunk64", 22)])
def test_full_size_proofs_pass_the_independent_verifier(hip_backend, tables, name, logn):
    """BASELINE configs[2]/[3] sizes: the CPU prover is too slow to compare against, but the verifier's
    cost does not depend on the trace length -- a 2^22..2^24-row proof from the MI355X must verify."""
    rc, mds = tables
    air = AIR.get_air(name)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 31337)
    params = PR.StarkParams(logn, logb=1, fri_logf=3, fri_final_log=5, n_queries=16)
    proof = PR.prove(air, tr, pub, params, hip_backend)
    del tr
    assert V.verify(proof, air.program(), rc, mds, V.expectation(params.to_dict()))
    bad = copy.deepcopy(proof)
    bad["evals"]["zw"][1][2] ^= 1
    with pytest.raises(V.Reject):
        V.verify(bad, air.program(), rc, mds, V.expectation(params.to_dict()))


@pytest.mark.parametrize("name,logn", [("fib", 6), ("perm", 8), ("wide32", 11), ("chunk16", 9), ("chunk64", 12)])
def test_constraint_program_interpreter_gives_the_same_proof(prover, hip_backend, cpu_backend, tables, name, logn):
    """zp_eval_quotient (the AIR as a data blob, interpreted on the GPU) == the generated kernel == the checker's CPU interpreter:
    whole proofs are byte-identical whichever evaluates the constraints"""
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    rc, mds = tables
    air = AIR.get_air(name)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 555 + logn)
    params = PR.StarkParams(logn, logb=1, fri_logf=3, fri_final_log=4, n_queries=5, pow_bits=6)
    be_prog = HipBackend(prover=prover, quotient="program")
    a = PR.proof_to_json(PR.prove(air, tr, pub, params, be_prog))
    assert a == PR.proof_to_json(PR.prove(air, tr, pub, params, hip_backend))
    assert a == PR.proof_to_json(PR.prove(air, tr, pub, params, cpu_backend))
    import json
    assert V.verify(json.loads(a), air.program(), rc, mds, V.expectation(params.to_dict()))


def test_eval_quotient_rejects_malformed_programs(prover):
    air = AIR.get_air("fib")
    good = air.program()
    M = 1 << 6
    d_cols, d_fixed, d_out = prover.alloc(2 * M), prover.alloc(2 * M), prover.alloc(3 * M)
    apow = [[1, 0, 0]] * len(air.constraints)
    args = lambda blob, pubs=(1, 2, 3): (blob, d_cols, d_fixed, 6, 1, list(pubs), apow, [1, 1], 49, 5, d_out)
    prover.eval_quotient(*args(good))
    for mutate in (lambda b: b.__setitem__(0, 7), lambda b: b.__setitem__(7, int(b[7]) + 1), lambda b: b.__setitem__(9, 99),
                   lambda b: b.__setitem__(12 + int(b[6]), 9), lambda b: b.__setitem__(12 + int(b[6]), int(b[12 + int(b[6])]) | (0xFFFF << 28))):
        bad = good.copy()
        mutate(bad)
        with pytest.raises(native.ZpError):
            prover.eval_quotient(*args(bad))
    with pytest.raises(native.ZpError):
        prover.eval_quotient(*args(good, pubs=(1, 2)))


def test_row_window_entry_points_match_the_whole_domain(prover):
    """zp_deep_quotient_rows / zp_eval_quotient_rows on a window (with its blow-up halo) == the same rows of the full call"""
    logm, logb, Wt = 10, 1, 8
    M, b = 1 << logm, 2
    air = AIR.get_air("wide8")
    cols = O.random_field((Wt, M), 901)
    q = O.random_field((3, M), 902)
    fixed = O.random_field((2, M), 903)
    z, zw, gamma = [O.random_field((3,), 904 + i).tolist() for i in range(3)]
    ev_z = O.random_field((Wt + 3, 3), 910)
    ev_zw = O.random_field((Wt, 3), 911)
    d_cols, d_q, d_fixed = prover.upload(cols), prover.upload(q), prover.upload(fixed)
    d_full = prover.alloc(3 * M)
    prover.deep_quotient(d_cols, Wt, d_q, 3, logm, Wt, z, zw, gamma, ev_z, ev_zw, 49, d_full)
    full = prover.download(d_full, (3, M))
    apow = [O.random_field((3,), 920 + k).tolist() for k in range(len(air.constraints))]
    pubs = [5, 6, 7, 8]
    d_qf = prover.alloc(3 * M)
    prover.eval_quotient(air.program(), d_cols, d_fixed, logm, logb, pubs, apow, [3, 9], 49, 12345, d_qf)
    qfull = prover.download(d_qf, (3, M))
    for row0, nrows in ((0, M // 4), (M // 4, M // 2), (3 * M // 4, M // 4)):
        d_a = prover.upload(cols[:, row0:row0 + nrows])
        d_b = prover.upload(q[:, row0:row0 + nrows])
        d_o = prover.alloc(3 * nrows)
        prover.deep_quotient_rows(d_a, Wt, nrows, d_b, 3, nrows, logm, row0, nrows, Wt, z, zw, gamma, ev_z, ev_zw, 49, d_o, nrows)
        assert (prover.download(d_o, (3, nrows)) == full[:, row0:row0 + nrows]).all()
        halo = np.concatenate([cols[:, row0:row0 + nrows], cols[:, [(row0 + nrows + k) % M for k in range(b)]]], axis=1)
        d_h = prover.upload(halo)
        d_f = prover.upload(fixed[:, row0:row0 + nrows])
        prover.eval_quotient_rows(air.program(), d_h, nrows + b, d_f, nrows, logm, logb, row0, nrows, pubs, apow, [3, 9], 49, 12345, d_o, nrows)
        assert (prover.download(d_o, (3, nrows)) == qfull[:, row0:row0 + nrows]).all()
    with pytest.raises(native.ZpError):      # a partial window without room for its halo
        prover.eval_quotient_rows(air.program(), d_cols, M // 2, d_fixed, M // 2, logm, logb, 0, M // 2, pubs, apow, [3, 9], 49, 12345, d_qf, M // 2)


def test_torch_side_paths_in_a_fresh_process():
    """four-step NTT through the layout kernels and the multi-GPU proof orchestration (stark/sharded.py, HIP ops, world size
    1) need torch CUDA tensors beside the library: torch has to initialise the GPU first, so they run as their own process"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_torch_checks.py")], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["ok"] and res["four_step_matches_plain_ntt"] and res["four_step_inverse_round_trip"]
    assert res["sharded_backend_world1_matches_plain_backend"]


@pytest.mark.parametrize("mode", ["kernel", "program"])
def test_degree_three_air_quotient_in_two_pieces(prover, cpu_backend, tables, mode):
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    rc, mds = tables
    air = AIR.get_air("cubic")
    tr, pub = AIR.cubic_witness(11, 9)
    params = PR.StarkParams(11, logb=1, fri_logf=3, fri_final_log=4, n_queries=6, pow_bits=6)
    gpu = PR.prove(air, tr, pub, params, HipBackend(prover=prover, quotient=mode))
    assert PR.proof_to_json(gpu) == PR.proof_to_json(PR.prove(air, tr, pub, params, cpu_backend))
    assert V.verify(gpu, air.program(), rc, mds, V.expectation(params.to_dict()))


@pytest.mark.parametrize("logn,logb", [(6, 1), (9, 2), (13, 1)])
def test_periodic_fixed_columns_gpu_matches_cpu_and_verifies(hip_backend, cpu_backend, tables, logn, logb):
    """sparse periodic fixed columns (constants with period 4, one entry per 8 rows, a public input at one row): the GPU
    interpreter reads ONE extended period per column (zp_fixed_columns), the CPU checker materialises whole columns; the
    quotients, the proofs (Python orchestration and zp_stark_prove) and the verdict of the independent verifier must agree"""
    rc, mds = tables
    air = AIR.periodic_air(logn)
    tr, pub = AIR.periodic_witness(logn, 5 + logn)
    params = PR.StarkParams(logn, logb, 2, 3, 6, pow_bits=4)
    p_cpu = PR.prove(air, tr, pub, params, cpu_backend)
    p_gpu = PR.prove(air, tr, pub, params, hip_backend)
    assert PR.proof_to_json(p_gpu) == PR.proof_to_json(p_cpu)
    assert V.verify(p_gpu, air.program(), rc, mds, V.expectation(params.to_dict()))
    d_tr = hip_backend.p.upload(tr)
    text = hip_backend.p.stark_prove(air.name, air.program(), d_tr, [int(v) for v in pub], logn, logb, 2, 3, 6, 4)
    assert text == PR.proof_to_json(p_cpu)
    bad = tr.copy()
    bad[2, 15] = (int(bad[2, 15]) + 1) % AIR.P                      # breaks S (a - b) = S c at one checkpoint row
    with pytest.raises(V.Reject):
        V.verify(PR.prove(air, bad, pub, params, hip_backend), air.program(), rc, mds, V.expectation(params.to_dict()))
