"""GPU tests of the BN254 MSM (N6): bit-exact against the definition-level oracle on small inputs,
group-law properties at larger sizes."""
import random

import numpy as np
import pytest

from oracle import naive_bn254 as B

pytestmark = pytest.mark.gpu


def limbs(v, n=8):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


@pytest.fixture(scope="module")
def table():
    rnd = random.Random(7)
    pts = [B.mul(B.G, rnd.randrange(1, B.R)) for _ in range(64)]
    assert all(B.on_curve(p) for p in pts)
    return pts


@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 64, 200, 1000])
def test_msm_matches_oracle(prover, table, n):
    rnd = random.Random(100 + n)
    pts = [table[rnd.randrange(len(table))] for _ in range(n)]
    scs = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    for i, v in enumerate([0, 1, B.R - 1, B.R, (1 << 254) - 1, 1 << 253][:n]):
        scs[i] = v
    if n <= 200:
        assert prover.msm_bn254(pts, scs) == B.msm(pts, scs)
    else:       # (the checker's double-and-add over 1000 points is half a minute of Python: per DISTINCT point of the 64-point table, as below)
        by_pt = {}
        for p, sc in zip(pts, scs):
            by_pt[p] = (by_pt.get(p, 0) + sc) % B.R
        assert prover.msm_bn254(pts, scs) == B.msm(list(by_pt), list(by_pt.values()))


def test_msm_in_several_runs_matches_oracle(prover, table):
    """n above the run size: partial sums of the runs are added on the host (forced here with 2^6-point runs)"""
    rnd = random.Random(4711)
    n = 300
    pts = [table[rnd.randrange(len(table))] for _ in range(n)]
    scs = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    prover.set_tuning("msm_chunk_log", 6)
    try:
        assert prover.msm_bn254(pts, scs) == B.msm(pts, scs)
    finally:
        prover.set_tuning("msm_chunk_log", 0)


@pytest.mark.parametrize("kind", ["ones", "tiny", "two_values", "top_heavy"])
def test_msm_skewed_scalars_take_the_heavy_bucket_path(prover, table, kind):
    """non-uniform scalars put thousands of points into one bucket: such buckets are summed by whole workgroups"""
    rnd = random.Random(31 + len(kind))
    n = 3000
    pts = [table[rnd.randrange(len(table))] for _ in range(n)]
    if kind == "ones":
        scs = [1] * n
    elif kind == "tiny":
        scs = [rnd.randrange(0, 4) for _ in range(n)]
    elif kind == "two_values":
        scs = [rnd.choice([B.R - 1, 12345678901234567890]) for _ in range(n)]
    else:   # random low bits, identical top bits: every window above the first is one heavy bucket
        scs = [(0x2F << 248) | (0xABCDEF << 100) | rnd.randrange(0, 1 << 20) for _ in range(n)]
    # the checker's double-and-add over 3000 points took a minute per case in pure Python: the points come from a small table, so the same sum
    # is taken per DISTINCT point first (sum_i s_i P_(t_i) = sum_t (sum_{i: t_i = t} s_i mod r) P_t) -- the definition plus linearity
    by_pt = {}
    for p, sc in zip(pts, scs):
        by_pt[p] = (by_pt.get(p, 0) + sc) % B.R
    assert prover.msm_bn254(pts, scs) == B.msm(list(by_pt), list(by_pt.values()))


def test_msm_g2_heavy_bucket_path(prover, table_g2):
    rnd = random.Random(5)
    n = 700
    pts = [table_g2[rnd.randrange(len(table_g2))] for _ in range(n)]
    scs = [rnd.randrange(1, 3) for _ in range(n)]
    assert prover.msm_bn254_g2(pts, scs) == B.msm_g2(pts, scs)


def test_msm_infinity_inputs_and_cancellation(prover, table):
    p = table[0]
    neg = (p[0], B.Q - p[1])
    assert prover.msm_bn254([p, neg], [5, 5]) is None                      # P - P = infinity
    assert prover.msm_bn254([(0, 0), p], [9, 3]) == B.mul(p, 3)            # (0,0) encodes infinity
    assert prover.msm_bn254([p, p, p], [1, 1, 1]) == B.mul(p, 3)           # doubling path inside a bucket
    assert prover.msm_bn254([p], [0]) is None


def test_msm_same_point_many_times(prover):
    # every point equal: exercises the doubling branch of the bucket accumulation; answer = (sum s) * G
    n = 1 << 14
    rnd = np.random.default_rng(3)
    scs = rnd.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    scs[:, 7] &= 0x0FFFFFFF
    pts = np.zeros((n, 16), dtype=np.uint32)
    pts[:, 0], pts[:, 8] = 1, 2
    total = sum(sum(int(scs[i, k]) << (32 * k) for k in range(8)) for i in range(n)) % B.R
    assert prover.msm_bn254_arrays(pts, scs) == B.mul(B.G, total)


def test_msm_large_table_property(prover, table):
    # 2^17 terms over a 64-point table: expected = sum_j (sum_{i: idx_i = j} s_i) * P_j
    n = 1 << 17
    rnd = np.random.default_rng(5)
    idx = rnd.integers(0, len(table), size=n)
    scs = rnd.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    scs[:, 7] &= 0x0FFFFFFF
    tab = np.array([limbs(p[0]) + limbs(p[1]) for p in table], dtype=np.uint32)
    pts = tab[idx]
    ints = [sum(int(scs[i, k]) << (32 * k) for k in range(8)) for i in range(n)]
    per = [0] * len(table)
    for i, j in enumerate(idx):
        per[j] = (per[j] + ints[i]) % B.R
    assert prover.msm_bn254_arrays(pts, scs) == B.msm(table, per)


@pytest.fixture(scope="module")
def table_g2():
    rnd = random.Random(77)
    pts = [B.mul_g2(B.G2, rnd.randrange(1, B.R)) for _ in range(16)]
    assert B.on_curve_g2(B.G2) and all(B.on_curve_g2(p) for p in pts)
    return pts


@pytest.mark.parametrize("n", [0, 1, 2, 5, 64, 300])
def test_msm_g2_matches_oracle(prover, table_g2, n):
    rnd = random.Random(900 + n)
    pts = [table_g2[rnd.randrange(len(table_g2))] for _ in range(n)]
    scs = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    for i, v in enumerate([0, 1, B.R - 1, B.R][:n]):
        scs[i] = v
    if n > 4:
        pts[4] = None                                     # infinity among the inputs
    assert prover.msm_bn254_g2(pts, scs) == B.msm_g2(pts, scs)


def test_msm_g2_cancellation_and_doubling(prover, table_g2):
    p = table_g2[0]
    neg = (p[0], ((-p[1][0]) % B.Q, (-p[1][1]) % B.Q))
    assert prover.msm_bn254_g2([p, neg], [5, 5]) is None
    assert prover.msm_bn254_g2([p] * 7, [1] * 7) == B.mul_g2(p, 7)      # same point in one bucket: the doubling branch


def test_golden_msm_vectors_through_cabi(prover, golden):
    """double-and-add vectors (oracle/naive_bn254.py -> tests/golden/vectors.json): infinity, zero and r-1 scalars, P + (-P)"""
    for case in golden["msm_g1"]:
        pts = [(int(x), int(y)) for x, y in case["points"]]
        got = prover.msm_bn254(pts, [int(v) for v in case["scalars"]])
        want = (int(case["sum"][0]), int(case["sum"][1]))
        assert (got or (0, 0)) == want
    for case in golden["msm_g2"]:
        pts = [((int(p[0][0]), int(p[0][1])), (int(p[1][0]), int(p[1][1]))) for p in case["points"]]
        got = prover.msm_bn254_g2(pts, [int(v) for v in case["scalars"]])
        assert got == ((int(case["sum"][0][0]), int(case["sum"][0][1])), (int(case["sum"][1][0]), int(case["sum"][1][1])))


# ---------------------------------------------------------------------------------------------------------------- the named seams
# Every comparison below is exact; the expectation is the oracle's double-and-add per DISTINCT point of a small table (the definition plus
# linearity, as above).  Sizes are the smallest that cross the seam.
def _g1_rows(table):
    return np.array([limbs(p[0]) + limbs(p[1]) for p in table], dtype=np.uint32)


def _g2_rows(table_g2):
    return np.array([limbs(p[0][0]) + limbs(p[0][1]) + limbs(p[1][0]) + limbs(p[1][1]) for p in table_g2], dtype=np.uint32)


def _scalar_rows(scs):
    return np.array([limbs(s) for s in scs], dtype=np.uint32).reshape(-1, 8)


def _width_for(n):
    """the window width msm_window_bits (csrc/msm.hip) picks for n points (its two loops and its floor of 6)"""
    c = 4
    while c < 16 and (1 << (c + 2)) <= n:
        c += 1
    while c < 20 and (1 << (c + 8)) <= n:
        c += 1
    return max(c, 6)


def _one_bucket(n, sign, ntable):
    """n points that all carry ONE scalar: 3 (one bucket of window 0 holds them all) or 2^(c+1) - 3, whose signed digits are (-3, +1)"""
    c = _width_for(n)
    assert _width_for(65 * 16384 + 1) == 16 and _width_for(1) == 6
    s = 3 if sign == "positive" else (1 << (c + 1)) - 3
    if sign == "negative":
        assert recode(s, c)[:3] == [-3, 1, 0]
    idx = np.random.default_rng(1000 + n).integers(0, ntable, size=n)
    scs = np.zeros((n, 8), dtype=np.uint32)
    scs[:, 0] = s
    return idx, scs, [int(k) * s % B.R for k in np.bincount(idx, minlength=ntable)]


def recode(s, c):
    """the signed window digits of s at bucket-index width c, lowest window first: u = s + K, digit = u_w - 2^c  (csrc/fq254.hpp, digit_key)"""
    cd = c + 1
    nwin = (258 + cd - 1) // cd
    u = s + sum(1 << (cd * w + cd - 1) for w in range(nwin))
    assert u < 1 << (cd * nwin)
    d = [((u >> (cd * w)) & ((1 << cd) - 1)) - (1 << c) for w in range(nwin)]
    assert sum(x << (cd * w) for w, x in enumerate(d)) == s
    return d


# 255 | 256 | 257: MSM_HEAVY;  16384 | 16385 | 32769: one, two and three MSM_HCHUNK chunks;  65 * 16384 + 1: 66 chunks, the strided loop of
# msm_heavy_combine_kernel;  1..5: the clamped prefetch indices of the two-point software pipeline
@pytest.mark.parametrize("sign", ["positive", "negative"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 16384, 16385, 32769, 65 * 16384 + 1])
def test_msm_one_bucket_of_every_seam_size(prover, table, n, sign):
    idx, scs, per = _one_bucket(n, sign, len(table))
    assert prover.msm_bn254_arrays(_g1_rows(table)[idx], scs) == B.msm(table, per)


@pytest.mark.parametrize("sign", ["positive", "negative"])
@pytest.mark.parametrize("n", [1, 2, 3, 256, 257, 16385])
def test_msm_g2_one_bucket_of_every_seam_size(prover, table_g2, n, sign):
    idx, scs, per = _one_bucket(n, sign, len(table_g2))
    assert prover.msm_bn254_g2_arrays(_g2_rows(table_g2)[idx], scs) == B.msm_g2(table_g2, per)


def signed_digit_scalars(c):
    """scalars made from digit vectors: each of -2^c, 2^c - 1, -1, 1, 0 in window 0, in the middle window and in the last but one; every window
    below the top at -2^c and at 2^c - 1 (carries of the bias addition across all nine words); the 256-bit extremes; 200 random ones"""
    cd = c + 1
    nwin = (258 + cd - 1) // cd
    places = (0, nwin // 2, nwin - 2)
    values = (-(1 << c), (1 << c) - 1, -1, 1, 0)
    vectors = []
    for w in places:
        for v in values:
            d = [0] * nwin
            d[w] = v
            vectors.append(d)
    vectors += [[-(1 << c)] * (nwin - 1) + [0], [(1 << c) - 1] * (nwin - 1) + [0]]
    scs = []
    for d in vectors:
        if sum(x << (cd * w) for w, x in enumerate(d)) < 0:
            d[nwin - 1] = 1
        scs.append(sum(x << (cd * w) for w, x in enumerate(d)))
    # conditions on the inputs (not compared with the GPU): every scalar is a 256-bit value and recodes to the digits it was made from
    assert all(0 <= s < 1 << 256 for s in scs)
    for s, d in zip(scs, vectors):
        assert recode(s, c) == d, (c, d)
    for w in places:
        for v in values:
            assert any(recode(s, c)[w] == v for s in scs), (c, w, v)
    assert any(all(x == -(1 << c) for x in recode(s, c)[:-1]) for s in scs) and any(all(x == (1 << c) - 1 for x in recode(s, c)[:-1]) for s in scs)
    rnd = random.Random(600 + c)
    return scs + [(1 << 256) - 1, 1 << 255, B.R - 1, B.R, B.R + 1] + [rnd.randrange(1 << 256) for _ in range(200)]


def _sum_per_point(idx, scs, ntable):
    per = [0] * ntable
    for i, s in zip(idx, scs):
        per[i] = (per[i] + s) % B.R
    return per


@pytest.mark.parametrize("c", [6, 7, 10, 11, 16, 17, 19, 20])
def test_msm_signed_digit_extremes_in_every_window(prover, table, c):
    """17 is the width of a 2^24-point run;  19 | 20: the 13 windows no longer fit the LDS budget of the tile kernels and are walked in passes of
    wgroup windows -- 7 and a ragged 6 at c = 19 (hi = 9), 4, 4, 4 and 1 at c = 20 (hi = 10)"""
    scs = signed_digit_scalars(c)
    rnd = random.Random(c)
    idx = [rnd.randrange(len(table)) for _ in scs]
    prover.set_tuning("msm_c", c)
    try:
        assert prover.msm_bn254_arrays(_g1_rows(table)[idx], _scalar_rows(scs)) == B.msm(table, _sum_per_point(idx, scs, len(table)))
    finally:
        prover.set_tuning("msm_c", 0)


@pytest.mark.parametrize("c", [6, 11, 16])
def test_msm_g2_signed_digit_extremes_in_every_window(prover, table_g2, c):
    scs = signed_digit_scalars(c)
    idx = [i % len(table_g2) for i in range(len(scs))]
    prover.set_tuning("msm_c", c)
    try:
        assert prover.msm_bn254_g2_arrays(_g2_rows(table_g2)[idx], _scalar_rows(scs)) == B.msm_g2(table_g2, _sum_per_point(idx, scs, len(table_g2)))
    finally:
        prover.set_tuning("msm_c", 0)


def _run_seams(msm_arrays, rows, neg_rows, tab, msm, mul, prover):
    """runs of 2^6 points, their sums added on the host (jac_add): a last run of one point; a run that repeats the one before (the host addition
    doubles); a run that is the negation of everything before it (the sum ends at infinity); a prefix that ends at infinity and a run added to it"""
    rnd = random.Random(64)
    idx = [rnd.randrange(len(tab)) for _ in range(64)]
    scs = [rnd.randrange(1 << 256) for _ in range(64)]
    per = _sum_per_point(idx, scs, len(tab))
    A = msm(tab, per)
    assert A is not None
    S, S2 = _scalar_rows(scs), _scalar_rows([2 * s % B.R for s in scs])
    last = rnd.randrange(len(tab))
    prover.set_tuning("msm_chunk_log", 6)
    try:
        # n = 129: two runs of A and a last run of one point
        per129 = [(2 * a + (B.R - 1 if t == last else 0)) % B.R for t, a in enumerate(per)]
        got = msm_arrays(np.concatenate([rows[idx], rows[idx], rows[[last]]]), np.concatenate([S, S, _scalar_rows([B.R - 1])]))
        assert got == msm(tab, per129)
        # n = 192: A, A again, then -2 A;  its prefix n = 128 is 2 A
        pts, sc = np.concatenate([rows[idx], rows[idx], neg_rows[idx]]), np.concatenate([S, S, S2])
        assert msm_arrays(pts, sc) is None
        assert msm_arrays(pts[:128], sc[:128]) == mul(A, 2)
        # n = 192: A, -A, A;  its prefix n = 128 ends at infinity, and the third run is added to infinity
        pts, sc = np.concatenate([rows[idx], neg_rows[idx], rows[idx]]), np.concatenate([S, S, S])
        assert msm_arrays(pts[:128], sc[:128]) is None
        assert msm_arrays(pts, sc) == A
    finally:
        prover.set_tuning("msm_chunk_log", 0)


def test_msm_run_seams(prover, table):
    _run_seams(prover.msm_bn254_arrays, _g1_rows(table), _g1_rows([(p[0], B.Q - p[1]) for p in table]), table, B.msm, B.mul, prover)


def test_msm_g2_run_seams(prover, table_g2):
    neg = [(p[0], ((-p[1][0]) % B.Q, (-p[1][1]) % B.Q)) for p in table_g2]
    _run_seams(prover.msm_bn254_g2_arrays, _g2_rows(table_g2), _g2_rows(neg), table_g2, B.msm_g2, B.mul_g2, prover)
