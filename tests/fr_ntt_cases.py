"""Shared by tests/test_fr_ntt_cases.py and tests/test_gpu_fr_ntt_shapes.py: what the sweep of the F_r transform and the QAP quotient
(csrc/ntt_bn254.hip: zp_ntt_bn254, zp_qap_quotient_bn254) stands on.  Pure Python, exact integers, no GPU.

  plan        `plan(logn)` RESTATES the pass rule of get_plan / run_ntt in csrc/ntt_bn254.hip (npass = ceil(logn / 8), the radices split
              evenly, R T = 1024 capped by N / R and, after the first pass, by P).  If that rule changes, re-read get_plan / run_ntt and
              restate it here: the size lists below are chosen so that every class (L, logT, first | later pass, inter-pass twiddle | last)
              of logn 1..28 is run by the GPU file, and tests/test_fr_ntt_cases.py asserts exactly that against THIS restatement.
  words       ints <-> u64[n][4] through int.to_bytes / np.frombuffer (Prover._fr_words loops per word: seconds at 2^20).
  references  for inputs with a handful of non-zero elements, by running powers (one modular product per term and output), never by a
              transform:  forward_window  y_k = sum_j x_j (g w^k)^(i_j);  forward_of_dense_window  the closed form of F_g applied to the DENSE
              Y = F(x):  (F_g Y)_k = sum_m Y_m (g w^k)^m = sum_j x_j sum_m (g w^(i_j + k))^m = sum_j x_j (g^N - 1) / (g w^(i_j + k) - 1).
  qap_case    sparse A, B (coefficients), P = A B, H = upper half of P, C = P_lo + P_hi:  A B - C = H (x^m - 1) exactly, H[m-1] = 0.
              qap_perturbed: C + D for a sparse D.  The interface's algorithm (evaluate on g <w>, divide by g^m - 1, interpolate m points)
              reduces A B - C - D modulo x^m - g^m; H x^m = H g^m there and deg D < m, so it returns H - D / (g^m - 1)."""
import functools
import random

import numpy as np

from oracle import naive as NV

FR = NV.FR

# the sizes tests/test_gpu_fr_ntt_shapes.py runs (2^26..2^28 are left out there: the classes of 25 again, on 2-8 GiB buffers)
DENSE_LOGN = tuple(range(0, 15))
DENSE_EXTRA_COSETS = (10, 13)           # dense sizes that also run g = r - 1 and g = the primitive 2N-th root
SPARSE_LOGN = tuple(range(15, 26))
QAP_LOGM = (1, 2, 3, 8, 9, 10, 16, 17)
WINDOW = 256


# ---- the plan rule, restated ----
def plan(logn):
    """[(L, logT, logP)] per pass, as get_plan / run_ntt (csrc/ntt_bn254.hip) choose them; logn = 0 has no pass"""
    if logn == 0:
        return []
    npass = (logn + 7) // 8
    out, logP = [], 0
    for i in range(npass):
        L = logn // npass + (1 if i < logn % npass else 0)
        logT = min(10 - L, logn - L)
        if i > 0:
            logT = min(logT, logP)
        out.append((L, logT, logP))
        logP += L
    return out


def classes(logns):
    """the pass classes (L, logT, "first" | "later", "tw" | "last") the sizes run"""
    out = set()
    for logn in logns:
        pl = plan(logn)
        for i, (L, logT, _) in enumerate(pl):
            out.add((L, logT, "first" if i == 0 else "later", "last" if i == len(pl) - 1 else "tw"))
    return out


def table_split(logn):
    """lb of the two-level tables: entry e = lo[e & (2^lb - 1)] * hi[e >> lb]"""
    return (logn + 1) // 2


# ---- words ----
def words(vals):
    """ints < 2^256 -> u64[n][4], little-endian words"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(a):
    raw = np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


# ---- references for sparse inputs ----
def forward_window(terms, logn, g, k0, count):
    """y_k = sum_j x_j (g w^k)^(i_j) for k = k0 .. k0 + count - 1; terms = [(i_j, x_j)]"""
    n, w = 1 << logn, NV.fr_root(logn)
    acc = [0] * count
    for i, x in terms:
        v = x * pow(g, i, FR) % FR * pow(w, i * k0 % n, FR) % FR
        s = pow(w, i, FR)
        for k in range(count):
            acc[k] += v
            v = v * s % FR
    return [a % FR for a in acc]


def batch_inverse(vals):
    """all inverses with one modular inversion"""
    pre, acc = [], 1
    for v in vals:
        assert v % FR != 0
        pre.append(acc)
        acc = acc * v % FR
    inv, out = pow(acc, FR - 2, FR), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % FR
        inv = inv * vals[i] % FR
    return out


def forward_of_dense_window(terms, logn, g, k0, count):
    """(F_g F x)_k for k = k0 .. k0 + count - 1, x given by its non-zero terms; needs g^N != 1 (then no g w^e is 1)"""
    n, w = 1 << logn, NV.fr_root(logn)
    top = (pow(g, n, FR) - 1) % FR
    assert top != 0, "g lies in the domain: the closed form does not apply"
    den = []
    for i, _ in terms:
        v, s = g * pow(w, (i + k0) % n, FR) % FR, w
        for _k in range(count):
            den.append((v - 1) % FR)
            v = v * s % FR
    inv = batch_inverse(den)
    return [sum(x * inv[j * count + k] for j, (_, x) in enumerate(terms)) % FR * top % FR for k in range(count)]


def reversed_scaled(terms, logn):
    """F(F(x)) = N x reversed: {position: value} of its non-zero elements"""
    n = 1 << logn
    return {(n - i) % n: n * x % FR for i, x in terms}


def dense_input(logn, rnd):
    """random, with x[0] = r - 1, x[N-1] = 0 and one element 1 (N >= 4; below that what fits, in this order of precedence)"""
    n = 1 << logn
    x = [rnd.randrange(FR) for _ in range(n)]
    if n >= 4:
        x[rnd.randrange(1, n - 1)] = 1
    x[n - 1] = 0
    x[0] = FR - 1
    return x


def random_coset(logn, rnd):
    """a shift outside the domain (so that forward_of_dense_window applies)"""
    while True:
        g = rnd.randrange(2, FR)
        if pow(g, 1 << logn, FR) != 1:
            return g


class SparseCase:
    """12..16 non-zero elements of a 2^logn buffer at the seams of the plan and of the two-level tables, a coset, the windows to compare"""

    def __init__(self, logn):
        rnd = random.Random(7000 + logn)
        n, lb = 1 << logn, table_split(logn)
        self.logn, self.n, self.lb = logn, n, lb
        pos = [0, 1, n - 1, n // 2, n >> plan(logn)[0][0], (1 << lb) - 1, 1 << lb, ((1 << (logn - lb)) - 1) << lb]
        pos = list(dict.fromkeys(pos))
        want = rnd.randrange(12, 17)
        while len(pos) < want:
            p = rnd.randrange(n)
            if p not in pos:
                pos.append(p)
        vals = [rnd.randrange(1, FR) for _ in pos]
        vals[0], vals[1] = FR - 1, 1
        self.terms = sorted(zip(pos, vals))
        self.g = random_coset(logn, rnd)
        wins = [0, n // 2 - WINDOW // 2, (1 << lb) - WINDOW // 2, n - WINDOW] + [rnd.randrange(n - WINDOW) for _ in range(4)]
        self.windows = sorted(set(wins))
        assert all(0 <= k and k + WINDOW <= n for k in self.windows)

    def as_dict(self):
        return dict(self.terms)


@functools.lru_cache(maxsize=None)
def sparse_case(logn):
    return SparseCase(logn)


# ---- the QAP quotient ----
def _sparse_poly(m, nterms, rnd):
    deg = {0, m - 1}
    while len(deg) < min(nterms, m):
        deg.add(rnd.randrange(m))
    return sorted((d, rnd.randrange(1, FR)) for d in deg)


class QapCase:
    """A B - C = H (x^m - 1) with everything known in closed form; *_terms are sparse coefficient lists [(degree, value)], *_ev the
    evaluations on <w> (running powers), h the m coefficients of H"""

    def __init__(self, logm, rnd):
        m = 1 << logm
        self.logm, self.m = logm, m
        nt = (3, 3) if logm >= 16 else (rnd.choice((3, 4)), rnd.choice((3, 4)))    # three each where every term costs 2^16 products
        self.a_terms, self.b_terms = _sparse_poly(m, nt[0], rnd), _sparse_poly(m, nt[1], rnd)
        prod = {}
        for i, a in self.a_terms:
            for j, b in self.b_terms:
                prod[i + j] = (prod.get(i + j, 0) + a * b) % FR
        h, c = {}, {}
        for d, v in prod.items():
            c[d % m] = (c.get(d % m, 0) + v) % FR          # P_lo + P_hi
            if d >= m:
                h[d - m] = v                               # the upper half; degree 2m - 1 does not occur
        self.h_terms = sorted((d, v) for d, v in h.items() if v)
        self.c_terms = sorted((d, v) for d, v in c.items() if v)
        self.h = [0] * m
        for d, v in self.h_terms:
            self.h[d] = v
        assert self.h[m - 1] == 0
        self.a_ev, self.b_ev, self.c_ev = (forward_window(t, logm, 1, 0, m) for t in (self.a_terms, self.b_terms, self.c_terms))


@functools.lru_cache(maxsize=None)
def qap_case(logm, seed=0):
    return QapCase(logm, random.Random(9000 + 100 * seed + logm))


def qap_cosets(logm, rnd):
    """7 (the product's, csrc/groth16.hip), the primitive 2m-th root (g^m = -1) and a random shift just below r"""
    m = 1 << logm
    while True:
        near = FR - 1 - rnd.randrange(1, 1 << 64)
        if pow(near, m, FR) != 1:
            break
    out = [7, NV.fr_root(logm + 1), near]
    assert pow(out[1], m, FR) == FR - 1 and all(pow(g, m, FR) != 1 for g in out)
    return out


def qap_perturbed(case, d_terms, g):
    """C + D in evaluations on <w>, and what the interface's algorithm returns for it on the coset g <w>: H - D / (g^m - 1)"""
    m = case.m
    d_ev = forward_window(d_terms, case.logm, 1, 0, m)
    c_ev = [(c + d) % FR for c, d in zip(case.c_ev, d_ev)]
    zinv = pow(pow(g, m, FR) - 1, FR - 2, FR)
    out = list(case.h)
    for deg, v in d_terms:
        out[deg] = (out[deg] - v * zinv) % FR
    return c_ev, out
