"""CPU test: the eight primitive 2^32-th roots that tests/test_gpu_ntt_forms.py drives the HIP transforms with.

The shift-only butterflies of csrc/ntt.hip use the fixed 16th root 2^12; a user's root enters as j0inv, the inverse mod 16 of
the j with (2^12)^j = w_16(user) (zpi_get_plan_role).  ROOT32_DEFAULT^k, k = 1, 3, .. 15, are eight valid roots whose forward
and inverse transforms each land in a different one of the eight odd classes.  The GPU module compares against the C oracle at
those roots, so here the C oracle is itself pinned at them: against the definition-level oracle/naive.py."""
import numpy as np

from oracle import naive as NV
from oracle import oracle as O

P = O.P
ROOTS = {k: pow(O.ROOT32_DEFAULT, k, P) for k in range(1, 16, 2)}
# the issue's table: k -> (forward j0inv, inverse j0inv)
CLASSES = {1: (5, 11), 3: (7, 9), 5: (1, 15), 7: (3, 13), 9: (13, 3), 11: (15, 1), 13: (9, 7), 15: (11, 5)}


def j0inv(root32, inverse):
    """the search of zpi_get_plan_role: j with (2^12)^j == w_16, then j^-1 mod 16"""
    w16 = pow(root32, 1 << 28, P)
    if inverse:
        w16 = pow(w16, P - 2, P)
    (j,) = [j for j in range(1, 16, 2) if pow(1 << 12, j, P) == w16]
    return pow(j, -1, 16)


def test_eight_roots_are_primitive_and_cover_the_eight_classes_each_way():
    assert pow(1 << 12, 8, P) == P - 1                       # 2^12 has order 16
    assert len(set(ROOTS.values())) == 8
    for k, r in ROOTS.items():
        assert 0 < r < P and pow(r, 1 << 31, P) == P - 1, k  # the check of zp_set_constants
        assert (j0inv(r, False), j0inv(r, True)) == CLASSES[k], k
        assert (j0inv(r, False) + j0inv(r, True)) % 16 == 0   # w_16^-1 = (2^12)^(-j): the two classes are negatives mod 16
    assert {c[0] for c in CLASSES.values()} == set(range(1, 16, 2))
    assert {c[1] for c in CLASSES.values()} == set(range(1, 16, 2))
    assert {j0inv(r, False) for r in ROOTS.values()} == set(range(1, 16, 2))
    assert {j0inv(r, True) for r in ROOTS.values()} == set(range(1, 16, 2))
    # the four roots k = 1, 3, 5, 7 meet all eight classes through forward and inverse together
    assert {c for k in (1, 3, 5, 7) for c in CLASSES[k]} == set(range(1, 16, 2))
    assert (j0inv(O.ROOT32_ALT, False), j0inv(O.ROOT32_ALT, True)) == (1, 15)


def test_oracle_matches_the_definition_at_every_root_class():
    """O.ntt / O.intt / O.lde / O.coset_scaled_coefficients at each of the eight roots against oracle/naive.py (O(n^2) sums and
    Horner evaluations), with the extreme field values in the input"""
    for k, r in ROOTS.items():
        for logn in (4, 6):
            n = 1 << logn
            x = O.random_field((2, n), 8800 + 16 * logn + k)
            x[0, :4] = np.array([0, P - 1, 1, 2 ** 32], dtype=np.uint64)
            xs = [[int(v) for v in col] for col in x]
            assert O.ntt(x, r).tolist() == [NV.ntt(c, r) for c in xs], (k, logn)
            assert O.intt(x, r).tolist() == [NV.intt(c, r) for c in xs], (k, logn)
            for logb, shift in ((1, 49), (2, 49), (1, 1)):
                assert O.lde(x, logb, shift, r).tolist() == [NV.lde(c, logb, shift, r) for c in xs], (k, logn, logb, shift)
            want = [[ci * pow(49, i, P) % P for i, ci in enumerate(NV.intt(c, r))] for c in xs]
            assert O.coset_scaled_coefficients(x, 49, r).tolist() == want, (k, logn)
    # the blocked form of the C transform (from 2^16 rows) against its plain loop at one non-default class each way
    x = O.random_field((1, 1 << 16), 8899)
    try:
        O.set_simple_ntt(True)
        plain = O.ntt(x, ROOTS[7]), O.intt(x, ROOTS[7])
    finally:
        O.set_simple_ntt(False)
    assert (O.ntt(x, ROOTS[7]) == plain[0]).all() and (O.intt(x, ROOTS[7]) == plain[1]).all()
