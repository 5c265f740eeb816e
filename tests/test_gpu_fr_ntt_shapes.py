"""zp_ntt_bn254 and zp_qap_quotient_bn254 (csrc/ntt_bn254.hip) at every pass shape of the plan, every coset path and every table seam,
against exact integers (tests/fr_ntt_cases.py, pinned to the checker by tests/test_fr_ntt_cases.py).  No tolerances.

  dense     every logn 0..14: forward, forward with coset, inverse, inverse with coset against oracle.naive.fr_ntt_fast, ALL N outputs.
  sparse    every logn 15..25, no dense host array: 12..16 non-zero elements at the seams (0, 1, N-1, N/2, N/R0, both sides of the split of
            the two-level tables, the last entry of their upper level), then
              1  Y = F(x)                     windows of 256 outputs against running-power sums
              2  F(Y) = N x reversed          the WHOLE buffer (dense data through every pass of the plain plan, every output checked)
              3  I(Y) = x                     the whole buffer
              4  Y_g = F_g(x) in windows;  I_g(Y_g) = x over the WHOLE buffer (dense data through out_mode 2)
              5  F_g(Y) in windows against the closed form (dense data through in_mode 1);  I_g of it = a device copy of Y, whole buffer
            Steps 3 and 5 are whole-buffer checks at EVERY size as well (no thinning was needed, see the times below).
            2^25 runs L = 7, 6, 6, 6 on 1 GiB of data + 1 GiB of scratch (+ 1 GiB for the copy of Y).  2^26..2^28 are left out: they run
            the pass classes of 2^25 again (tests/test_fr_ntt_cases.py shows the classes complete without them) on 2-8 GiB buffers.
            The upper level of the two-level tables has 2^(logn - lb) entries: 2^12 at 2^24 and 2^25, the largest index this file reaches
            (an index cut to 12 bits goes unseen below 2^26; one cut to 11 bits fails 2^24 and 2^25).
  qap       logm 1, 2, 3, 8, 9, 10, 16, 17: all m coefficients of H for three cosets, d_b and d_c on return (= B, C on g <w>), and an
            unsatisfied system (H - D / (g^m - 1)).
  caches    sizes, directions and cosets interleaved on one ctx and on a second ctx of the same device.
  refusals  each leaves the buffers bit-identical.

Wall-clock on an MI355X (pytest --durations, call phase, one run of the 39 tests of this file: about 3.5 s in all, setup included):
  dense    2^14 0.31 s, 2^13 0.29 s (three cosets), 2^12 0.07 s, below that 0.03 s or less -- the time is the checker's recursion
  sparse   2^25 0.36 s, 2^24 0.21 s, 2^23 0.13 s, 2^15..2^22 0.05-0.08 s -- the whole-buffer checks come down in 32 MiB pieces
           through page-locked memory; with every test far below 5 s, steps 3 and 5 were not thinned at any size
  qap      2^17 0.50 s, 2^16 0.25 s, up to 2^10 0.01 s; the unsatisfied system 0.14 s at 2^16 -- the time is the running-power evaluation
  caches   0.09 s;  refusals below 0.005 s"""
import random

import numpy as np
import pytest

import fr_ntt_cases as FC
from oracle import naive as NV

pytestmark = pytest.mark.gpu
FR = NV.FR
W = FC.WINDOW
PIECE = 1 << 20                        # elements per download of a whole-buffer check (32 MiB)


def _first_bad(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return "first differing elements %s of %d" % (bad[:4].tolist(), len(bad))


def _same(got, want_ints, what):
    want = FC.words(want_ints)
    assert got.shape == want.shape
    assert (got == want).all(), "%s: %s" % (what, _first_bad(got, want))


@pytest.fixture(scope="module")
def pieces(prover):
    """two page-locked host buffers for the piecewise downloads"""
    arr = prover.host_array((2, PIECE, 4))
    yield arr
    prover.release_host_array(arr)


def _fetch(prover, host, d, off, cnt):
    """elements off .. off + cnt of the device buffer into host[:cnt]"""
    out = host[:cnt]
    prover._chk(prover.lib.zp_d2h(prover.ctx, out.ctypes.data, d.ptr + 32 * off, 32 * cnt))
    return out


# ---- a. dense, every output ----
@pytest.mark.parametrize("logn", FC.DENSE_LOGN)
def test_dense_all_forms_every_output(prover, logn):
    rnd = random.Random(500 + logn)
    n = 1 << logn
    x = FC.dense_input(logn, rnd)
    if n >= 4:
        assert x[0] == FR - 1 and x[n - 1] == 0 and 1 in x
    cosets = [FC.random_coset(logn, rnd)]
    if logn in FC.DENSE_EXTRA_COSETS:   # also g = r - 1 and the primitive 2N-th root
        cosets += [FR - 1, NV.fr_root(logn + 1)]
    xw = FC.words(x)
    d = prover.alloc(4 * n)

    def run(inverse, g):
        prover.h2d(d, xw)
        prover.ntt_bn254(d, logn, inverse, g)
        return prover.download(d, (n, 4))

    try:
        _same(run(False, None), NV.fr_ntt_fast(x), "forward")
        _same(run(True, None), NV.fr_ntt_fast(x, inverse=True), "inverse")
        for g in cosets:
            _same(run(False, g), NV.fr_ntt_fast(x, coset=g), "forward, coset %x" % g)
            _same(run(True, g), NV.fr_ntt_fast(x, inverse=True, coset=g), "inverse, coset %x" % g)
        if logn == 0:                  # one point: the identity in every form
            for inverse in (False, True):
                for g in (None, 1, cosets[0], FR - 1):
                    assert (run(inverse, g) == xw).all()
    finally:
        d.free()


# ---- b. sparse input, composed transforms ----
def _write_sparse(prover, d, cs):
    prover.memset(d, 0, 32 * cs.n)
    for i, v in cs.terms:
        prover.h2d(d.offset(4 * i), FC.words([v]))


def _windows(prover, d, cs, ref, what):
    for k0 in cs.windows:
        got = prover.download(d, (W, 4), 4 * k0)
        _same(got, ref(k0), "%s, outputs %d..%d" % (what, k0, k0 + W - 1))


def _whole(prover, host, d, n, expected, what):
    """the buffer holds `expected` ({position: value}) and zero everywhere else"""
    todo = sorted(expected.items())
    for off in range(0, n, PIECE):
        cnt = min(PIECE, n - off)
        a = _fetch(prover, host, d, off, cnt)
        while todo and todo[0][0] < off + cnt:
            pos, val = todo.pop(0)
            assert FC.ints(a[pos - off]) == [val], "%s: element %d" % (what, pos)
            a[pos - off] = 0
        if np.count_nonzero(a):
            bad = np.flatnonzero(a.any(axis=1))
            raise AssertionError("%s: %d elements of %d..%d should be zero, first %s" % (what, len(bad), off, off + cnt - 1, (bad[:4] + off).tolist()))
    assert not todo


def _whole_equal(prover, host, d, d_ref, n, what):
    for off in range(0, n, PIECE):
        cnt = min(PIECE, n - off)
        a, b = _fetch(prover, host[0], d, off, cnt), _fetch(prover, host[1], d_ref, off, cnt)
        assert np.array_equal(a, b), "%s, elements %d..%d: %s" % (what, off, off + cnt - 1, _first_bad(a, b))


@pytest.mark.parametrize("logn", FC.SPARSE_LOGN)
def test_sparse_input_through_every_composition(prover, pieces, logn):
    cs = FC.sparse_case(logn)
    n, g, terms, x = cs.n, cs.g, cs.terms, cs.as_dict()
    d, dy = prover.alloc(4 * n), prover.alloc(4 * n)
    try:
        _write_sparse(prover, d, cs)
        # 1
        prover.ntt_bn254(d, logn)
        _windows(prover, d, cs, lambda k0: FC.forward_window(terms, logn, 1, k0, W), "F(x)")
        prover.d2d(dy, d, 32 * n)
        # 2
        prover.ntt_bn254(d, logn)
        _whole(prover, pieces[0], d, n, FC.reversed_scaled(terms, logn), "F(F(x)) = N x reversed")
        # 3
        prover.d2d(d, dy, 32 * n)
        prover.ntt_bn254(d, logn, True)
        _whole(prover, pieces[0], d, n, x, "I(F(x)) = x")
        # 4
        prover.ntt_bn254(d, logn, False, g)
        _windows(prover, d, cs, lambda k0: FC.forward_window(terms, logn, g, k0, W), "F_g(x)")
        prover.ntt_bn254(d, logn, True, g)
        _whole(prover, pieces[0], d, n, x, "I_g(F_g(x)) = x")
        # 5
        prover.d2d(d, dy, 32 * n)
        prover.ntt_bn254(d, logn, False, g)
        _windows(prover, d, cs, lambda k0: FC.forward_of_dense_window(terms, logn, g, k0, W), "F_g(F(x))")
        prover.ntt_bn254(d, logn, True, g)
        _whole_equal(prover, pieces, d, dy, n, "I_g(F_g(Y)) = Y")
    finally:
        d.free()
        dy.free()


# ---- c. the QAP quotient ----
def _qap(prover, bufs, logm, g):
    cw = FC.words([g])
    prover._chk(prover.lib.zp_qap_quotient_bn254(prover.ctx, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, logm, cw.ctypes.data))


@pytest.mark.parametrize("logm", FC.QAP_LOGM)
def test_qap_quotient_every_coefficient_and_the_coset_evaluations(prover, logm):
    cs = FC.qap_case(logm)
    m, rnd = cs.m, random.Random(600 + logm)
    ev = [FC.words(v) for v in (cs.a_ev, cs.b_ev, cs.c_ev)]
    hw = FC.words(cs.h)
    bufs = [prover.alloc(4 * m) for _ in range(3)]
    if m <= 1 << 10:
        wins = [(0, m)]                                                    # d_b, d_c: the whole buffer
    else:
        wins = [(k0, W) for k0 in sorted({0, m // 2 - W // 2, m - W, rnd.randrange(m - W), rnd.randrange(m - W)})]
    try:
        for g in FC.qap_cosets(logm, rnd):
            for b, v in zip(bufs, ev):
                prover.h2d(b, v)
            _qap(prover, bufs, logm, g)
            got = prover.download(bufs[0], (m, 4))
            assert (got == hw).all(), "H, coset %x: %s" % (g, _first_bad(got, hw))
            for name, b, terms in (("B", bufs[1], cs.b_terms), ("C", bufs[2], cs.c_terms)):
                for k0, cnt in wins:
                    _same(prover.download(b, (cnt, 4), 4 * k0), FC.forward_window(terms, logm, g, k0, cnt),
                          "%s on the coset %x, points %d..%d" % (name, g, k0, k0 + cnt - 1))
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("logm", [2, 9, 16])
def test_qap_quotient_of_an_unsatisfied_system(prover, logm):
    """C + D: the interpolation of (A B - C - D) / (g^m - 1) on g <w>, which is H - D / (g^m - 1) and depends on g"""
    cs = FC.qap_case(logm)
    m, rnd = cs.m, random.Random(700 + logm)
    d_terms = sorted({0: rnd.randrange(1, FR), m - 1: rnd.randrange(1, FR), rnd.randrange(1, m - 1): FR - 1}.items())
    g7, _, near = FC.qap_cosets(logm, rnd)
    bufs = [prover.alloc(4 * m) for _ in range(3)]
    results = []
    try:
        for g in (g7, near):
            c_ev, want = FC.qap_perturbed(cs, d_terms, g)
            assert want[m - 1] != 0
            for b, v in zip(bufs, (cs.a_ev, cs.b_ev, c_ev)):
                prover.h2d(b, FC.words(v))
            _qap(prover, bufs, logm, g)
            got = prover.download(bufs[0], (m, 4))
            _same(got, want, "H - D / (g^m - 1), coset %x" % g)
            results.append(got)
        assert (results[0] != results[1]).any()
    finally:
        for b in bufs:
            b.free()


# ---- d. the process-wide caches ----
def _cache_round(p, inputs, cosets):
    """sizes a, b, a; at each forward and inverse with cosets g1, g2, g1 and none -> {(visit, logn, inverse, coset slot): words}"""
    out = {}
    for visit, logn in enumerate((6, 11, 6)):
        n = 1 << logn
        d = p.alloc(4 * n)
        for slot, g in enumerate((cosets[0], cosets[1], cosets[0], None)):
            for inverse in (False, True):
                p.h2d(d, inputs[logn])
                p.ntt_bn254(d, logn, inverse, g)
                out[(visit, logn, inverse, slot)] = p.download(d, (n, 4))
        d.free()
    return out


def test_caches_keep_sizes_directions_cosets_and_contexts_apart(prover):
    from eigen_zeth_amd.native import Prover
    rnd = random.Random(800)
    x = {logn: [rnd.randrange(FR) for _ in range(1 << logn)] for logn in (6, 11)}
    inputs = {logn: FC.words(v) for logn, v in x.items()}
    cosets = (rnd.randrange(2, FR), FR - 1 - rnd.randrange(1 << 40))
    first = _cache_round(prover, inputs, cosets)
    for (visit, logn, inverse, slot), got in first.items():
        if visit == 0 or logn == 11:                                       # the first results are right ...
            g = (cosets[0], cosets[1], cosets[0], 1)[slot]
            _same(got, NV.fr_ntt_fast(x[logn], inverse=inverse, coset=g), "2^%d inverse=%d coset slot %d" % (logn, inverse, slot))

    def same_as_first(res, what):
        for key, got in res.items():
            ref = first[(0 if key[1] == 6 else 1, key[1], key[2], 0 if key[3] == 2 else key[3])]
            assert (got == ref).all(), "%s: visit %d, 2^%d, inverse=%d, coset slot %d: %s" % ((what,) + key + (_first_bad(got, ref),))

    same_as_first(first, "first ctx")                                      # ... and every later one equals them
    second = Prover(0)
    try:
        same_as_first(_cache_round(second, inputs, cosets), "second ctx")
        same_as_first(_cache_round(prover, inputs, cosets), "first ctx while the second lives")
    finally:
        second.close()
    same_as_first(_cache_round(prover, inputs, cosets), "first ctx after the second is closed")


# ---- e. refusals ----
def test_refusals_leave_the_buffers_untouched(prover):
    from eigen_zeth_amd.native import ZpError
    rnd = random.Random(900)
    logm, m = 4, 16
    data = [FC.words([rnd.randrange(FR) for _ in range(m)]) for _ in range(3)]
    bufs = [prover.upload(v.reshape(-1)) for v in data]
    lib, ctx = prover.lib, prover.ctx

    def refused(call, what):
        with pytest.raises(ZpError):
            prover._chk(call())
        for b, v in zip(bufs, data):
            assert (prover.download(b, (m, 4)) == v).all(), "%s changed a buffer" % what

    def ntt(ptr, logn, inverse, g):
        cw = FC.words([g]) if g is not None else None
        return lambda: lib.zp_ntt_bn254(ctx, ptr, logn, inverse, cw.ctypes.data if cw is not None else None)

    def qap(ptrs, lg, g):
        cw = FC.words([g]) if g is not None else None
        return lambda: lib.zp_qap_quotient_bn254(ctx, ptrs[0], ptrs[1], ptrs[2], lg, cw.ctypes.data if cw is not None else None)

    ptrs = [b.ptr for b in bufs]
    try:
        for inverse in (0, 1):
            refused(ntt(ptrs[0], -1, inverse, None), "logn = -1")
            refused(ntt(ptrs[0], 29, inverse, None), "logn = 29")
            refused(ntt(ptrs[0], logm, inverse, FR), "coset = r")
            refused(ntt(ptrs[0], logm, inverse, (1 << 256) - 1), "coset = 2^256 - 1")
            refused(ntt(ptrs[0], logm, inverse, 0), "coset = 0")
            refused(ntt(None, logm, inverse, None), "null data")
            refused(ntt(None, 0, inverse, 7), "null data at logn = 0")
        refused(qap(ptrs, 0, 7), "QAP with logm = 0")
        refused(qap(ptrs, -1, 7), "QAP with logm = -1")
        refused(qap(ptrs, 29, 7), "QAP with logm = 29")
        w = NV.fr_root(logm)
        refused(qap(ptrs, logm, pow(w, 3, FR)), "QAP with g = w^3")
        refused(qap(ptrs, logm, w), "QAP with g = w")
        refused(qap(ptrs, logm, 1), "QAP with g = 1")
        for lg in (1, 2, logm):
            refused(qap(ptrs, lg, FR - 1), "QAP with g = r - 1 at logm = %d" % lg)
        refused(qap(ptrs, logm, 0), "QAP with g = 0")
        refused(qap(ptrs, logm, FR), "QAP with g = r")
        refused(qap(ptrs, logm, (1 << 256) - 1), "QAP with g = 2^256 - 1")
        refused(qap(ptrs, logm, None), "QAP with a null coset")
        for k in range(3):
            refused(qap(ptrs[:k] + [None] + ptrs[k + 1:], logm, 7), "QAP with null buffer %d" % k)
        # nothing above left the ctx or the caches in a bad state
        prover.ntt_bn254(bufs[0], logm, False, 7)
        _same(prover.download(bufs[0], (m, 4)), NV.fr_ntt_fast(FC.ints(data[0]), coset=7), "a transform after the refusals")
    finally:
        for b in bufs:
            b.free()
