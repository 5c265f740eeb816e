"""The helpers of tests/fr_ntt_cases.py, on the CPU: the sparse-input references and the closed-form QAP systems are pinned to the
definition-level checker (oracle/naive.py: fr_ntt, fr_ntt_fast, qap_quotient) at small sizes, and the sizes the GPU file
(tests/test_gpu_fr_ntt_shapes.py) runs are shown to reach every pass class of the plan rule -- so that the device tests stand on references
that are what they claim to be."""
import random

import numpy as np
import pytest

import fr_ntt_cases as FC
from eigen_zeth_amd.native import Prover
from oracle import naive as NV

FR = NV.FR


def _dense(terms, n):
    x = [0] * n
    for i, v in terms:
        x[i] = v
    return x


def _cosets(logn, rnd):
    return [7, NV.fr_root(logn + 1), FR - 2, FC.random_coset(logn, rnd)]


def test_plan_classes_and_coverage():
    every = FC.classes(range(1, 29))
    assert len(every) == 21
    assert FC.classes(range(1, 26)) == every                              # nothing new from 2^26 up
    ran = FC.classes(FC.DENSE_LOGN + FC.SPARSE_LOGN)
    assert ran == every, "classes no GPU test runs: %s" % sorted(every - ran)
    assert FC.DENSE_LOGN == tuple(range(0, 15)) and FC.SPARSE_LOGN == tuple(range(15, 26))
    assert len(FC.DENSE_EXTRA_COSETS) == 2 and set(FC.DENSE_EXTRA_COSETS) <= set(FC.DENSE_LOGN)
    # the facts the size lists were chosen by
    assert FC.plan(10) == [(5, 5, 0), (5, 5, 5)]
    assert [logn for logn in range(1, 29) if (5, 5, "first", "tw") in FC.classes([logn])] == [10]
    assert [logn for logn in range(1, 29) if (8, 2, "later", "tw") in FC.classes([logn])] == [23, 24]
    assert [logn for logn in range(1, 29) if (7, 3, "later", "last") in FC.classes([logn])] == [14, 15, 21, 22, 23, 28]
    assert [p[0] for p in FC.plan(25)] == [7, 6, 6, 6] and [p[0] for p in FC.plan(24)] == [8, 8, 8]
    for L in (1, 2, 4, 6, 7):
        assert FC.classes([L]) == {(L, 0, "first", "last")}
    for logn in range(1, 29):
        pl = FC.plan(logn)
        assert sum(p[0] for p in pl) == logn and all(1 <= L <= 8 and 0 <= logT and L + logT <= 10 for L, logT, _ in pl)
        assert all(logT <= logP for _, logT, logP in pl[1:]) and all(logT <= logn - L for L, logT, _ in pl)


def test_words_round_trip_and_match_the_binding():
    rnd = random.Random(1)
    vals = [0, 1, FR - 1, (1 << 256) - 1, 1 << 64, (1 << 64) - 1, 1 << 192] + [rnd.randrange(1 << 256) for _ in range(50)]
    w = FC.words(vals)
    assert w.dtype == np.uint64 and w.shape == (len(vals), 4) and w.flags.writeable
    assert (w == Prover._fr_words(vals)).all()
    assert FC.ints(w) == vals == Prover._fr_ints(w)
    assert FC.ints(w[3]) == [vals[3]] and FC.ints(w[::2]) == vals[::2]    # one row, a strided view


def test_batch_inverse():
    rnd = random.Random(2)
    vals = [1, FR - 1, 2] + [rnd.randrange(1, FR) for _ in range(20)]
    assert [v * i % FR for v, i in zip(vals, FC.batch_inverse(vals))] == [1] * len(vals)


@pytest.mark.parametrize("logn", [1, 2, 5, 9])
def test_forward_window_is_the_transform(logn):
    rnd = random.Random(10 + logn)
    n = 1 << logn
    d = {rnd.randrange(n): rnd.randrange(1, FR) for _ in range(6)}
    d[0], d[n - 1] = FR - 1, 5
    terms = sorted(d.items())
    x = _dense(terms, n)
    for g in [1] + _cosets(logn, rnd):
        ref = NV.fr_ntt_fast(x, coset=g)
        assert FC.forward_window(terms, logn, g, 0, n) == ref
        if logn <= 5:
            assert ref == NV.fr_ntt(x, coset=g)
        k0 = rnd.randrange(n)
        cnt = min(7, n - k0)
        assert FC.forward_window(terms, logn, g, k0, cnt) == ref[k0:k0 + cnt]


@pytest.mark.parametrize("logn", [1, 2, 5, 9])
def test_forward_of_dense_window_and_double_transform(logn):
    rnd = random.Random(20 + logn)
    n = 1 << logn
    terms = sorted({rnd.randrange(n): rnd.randrange(1, FR) for _ in range(5)}.items())
    x = _dense(terms, n)
    y = NV.fr_ntt_fast(x)
    yy = NV.fr_ntt_fast(y)
    assert yy == [n * x[-k % n] % FR for k in range(n)]                   # F(F(x))_k = N x_(-k mod N)
    assert _dense(FC.reversed_scaled(terms, logn).items(), n) == yy
    assert NV.fr_ntt_fast(y, inverse=True) == x
    for g in _cosets(logn, rnd):
        ref = NV.fr_ntt_fast(y, coset=g)
        assert FC.forward_of_dense_window(terms, logn, g, 0, n) == ref
        k0 = rnd.randrange(n)
        cnt = min(5, n - k0)
        assert FC.forward_of_dense_window(terms, logn, g, k0, cnt) == ref[k0:k0 + cnt]
        assert NV.fr_ntt_fast(ref, inverse=True, coset=g) == y
    with pytest.raises(AssertionError):
        FC.forward_of_dense_window(terms, logn, NV.fr_root(logn), 0, 1)     # in-domain shift: no closed form


def test_sparse_cases_sit_on_the_seams():
    for logn in FC.SPARSE_LOGN:
        cs = FC.sparse_case(logn)
        n, lb, d = cs.n, cs.lb, cs.as_dict()
        assert 12 <= len(cs.terms) <= 16 and len(d) == len(cs.terms) and all(0 <= i < n and 0 < v < FR for i, v in cs.terms)
        for p in (0, 1, n - 1, n // 2, n >> FC.plan(logn)[0][0], (1 << lb) - 1, 1 << lb, ((1 << (logn - lb)) - 1) << lb):
            assert p in d
        assert FR - 1 in d.values() and 1 in d.values()
        assert pow(cs.g, n, FR) != 1
        assert {0, n // 2 - 128, (1 << lb) - 128, n - 256} <= set(cs.windows) and len(cs.windows) >= 6
        assert FC.sparse_case(logn) is cs                                  # made once, shared


@pytest.mark.parametrize("logm", [1, 2, 5, 9])
def test_qap_case_is_a_satisfied_system_with_the_stated_quotient(logm):
    cs = FC.qap_case(logm)
    m = cs.m
    assert {0, m - 1} <= {d for d, _ in cs.a_terms} and {0, m - 1} <= {d for d, _ in cs.b_terms}
    assert len(cs.a_terms) in (min(3, m), min(4, m)) and len(cs.b_terms) in (min(3, m), min(4, m))
    A, B, Cc = (_dense(t, m) for t in (cs.a_terms, cs.b_terms, cs.c_terms))
    assert cs.a_ev == NV.fr_ntt_fast(A) and cs.b_ev == NV.fr_ntt_fast(B) and cs.c_ev == NV.fr_ntt_fast(Cc)
    assert cs.c_ev == [a * b % FR for a, b in zip(cs.a_ev, cs.b_ev)]
    assert any(cs.h) and cs.h[m - 1] == 0
    if logm <= 5:
        assert NV.qap_quotient(cs.a_ev, cs.b_ev, cs.c_ev) == cs.h
    z = random.Random(logm).randrange(FR)                                  # A B - C = H (x^m - 1) at a random point
    ev = lambda co: NV.poly_eval_mod(co, z, FR)
    assert (ev(A) * ev(B) - ev(Cc)) % FR == ev(cs.h) * (pow(z, m, FR) - 1) % FR


@pytest.mark.parametrize("logm", [1, 2, 5, 9])
def test_qap_perturbed_is_what_the_coset_algorithm_returns(logm):
    """the algorithm of zp_qap_quotient_bn254, step by step with the checker's transforms, on an UNSATISFIED system"""
    cs = FC.qap_case(logm)
    m, rnd = cs.m, random.Random(30 + logm)
    d_terms = sorted({0: rnd.randrange(1, FR), m - 1: rnd.randrange(1, FR), rnd.randrange(m): FR - 1}.items())
    for g in FC.qap_cosets(logm, rnd):
        c_ev, want = FC.qap_perturbed(cs, d_terms, g)
        assert c_ev != cs.c_ev and want != cs.h
        on_coset = [NV.fr_ntt_fast(NV.fr_ntt_fast(v, inverse=True), coset=g) for v in (cs.a_ev, cs.b_ev, c_ev)]
        zinv = pow(pow(g, m, FR) - 1, FR - 2, FR)
        q = [(a * b - c) * zinv % FR for a, b, c in zip(*on_coset)]
        assert NV.fr_ntt_fast(q, inverse=True, coset=g) == want
        # ... and with D = 0 the same steps give H itself
        on_coset[2] = NV.fr_ntt_fast(NV.fr_ntt_fast(cs.c_ev, inverse=True), coset=g)
        q = [(a * b - c) * zinv % FR for a, b, c in zip(*on_coset)]
        assert NV.fr_ntt_fast(q, inverse=True, coset=g) == cs.h
        assert on_coset[1] == FC.forward_window(cs.b_terms, logm, g, 0, m)   # what d_b holds on return
