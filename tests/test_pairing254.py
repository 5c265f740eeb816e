"""The pairing arithmetic of csrc/pairing254.hpp, function by function, on the host.

tests/native/pairing254_check.cpp runs each function on a case file and writes every word it returns; it judges nothing.  Every expectation is made
here from the checker (oracle/bn254_pairing.py, oracle/naive_bn254.py) and Python integers: products, inverses and Frobenius maps against
BP.f_mul / f_inv / f_pow(., q^k) after the change to the flat basis, the final exponentiation alone against BP.final_exp on random elements (the
check that the exponent is exactly (q^12 - 1)/r), whole pairings against BP.pairing and e(G1, G2)^(ab), the subgroup test against [r]Q = O on
multiples of the generator, on a twist point outside G2 and on the twist points of the reference's key.  Field operands include 0, 1, q - 1 and
the limb-boundary values of tests/test_fq254.py (fq_operands: the set its own F_q cases use).

The program is built plainly and as a stand-alone program under ASan + UBSan."""
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import bn254_pairing as BP
from oracle import naive_bn254 as B
from test_field_corners import CSRC, NATIVE, ROOT
from test_fq254 import fq_operands

Q, R = B.Q, B.R
RR = 1 << 261
RINV = pow(RR, -1, Q)
MASK29 = (1 << 29) - 1
SAN = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
OPS = ["fq_inv", "fq2_inv", "fq12_mul", "fq12_sqr", "fq12_mul_line", "fq12_inv", "fq12_conj", "fq12_frob1", "fq12_frob2", "fq12_frob3",
       "fq12_final_exp", "pairing", "g2_checks"]
CASE_WORDS, OUT_WORDS = 218, 205     # u32 op, flags, x[2][108]  /  u32 r[108], flag, w[96]
SRC = os.path.join(NATIVE, "pairing254_check.cpp")


def mont(v):
    m = v * RR % Q
    return [(m >> (29 * i)) & MASK29 for i in range(9)]


def unmont(l):
    assert all(0 <= x <= MASK29 for x in l), "limbs not normalised"
    m = sum(x << (29 * i) for i, x in enumerate(l))
    assert m < Q, "value not reduced"
    return m * RINV % Q


def words(v, n=8):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


def unwords(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w))


def flat_limbs(a):
    return [x for c in a for x in mont(c)]


def g1_words(p):
    return [0] * 16 if p is None else words(p[0]) + words(p[1])


def g2_words(p):
    return [0] * 32 if p is None else words(p[0][0]) + words(p[0][1]) + words(p[1][0]) + words(p[1][1])


def f2_sqrt(a):
    """a square root in F_q2 (q = 3 mod 4), or None"""
    f2_pow = lambda x, e: B.f2_mul(f2_pow(B.f2_mul(x, x), e >> 1), x if e & 1 else (1, 0)) if e else (1, 0)
    a1 = f2_pow(a, (Q - 3) // 4)
    alpha = B.f2_mul(B.f2_mul(a1, a1), a)
    x0 = B.f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        r = B.f2_mul((0, 1), x0)
    else:
        r = B.f2_mul(f2_pow(B.f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    return r if B.f2_mul(r, r) == (a[0] % Q, a[1] % Q) else None


def off_subgroup_point():
    """the twist point with x = 2 + u: on y^2 = x^3 + 3/(9 + u), and [r]Q != O"""
    x = (2, 1)
    y = f2_sqrt(B.f2_add(B.f2_mul(B.f2_mul(x, x), x), B.B2))
    assert y is not None
    p = (x, y)
    assert B.on_curve_g2(p) and B.mul_g2(p, R) is not None
    return p


def ref_vk_points():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_vk.json")))
    g1 = [(int(p[0]), int(p[1])) for p in d["g1"]]
    g2 = [((int(p[0]), int(p[1])), (int(p[2]), int(p[3]))) for p in d["g2_words"]]
    return g1, g2


_E1 = []


def e1():
    """e(G1, G2), once per session"""
    if not _E1:
        _E1.append(BP.pairing(B.G2, B.G))
    return _E1[0]


class Cases:
    def __init__(self):
        self.rows = []

    def add(self, op, x0=(), x1=(), flags=0, r=None, flag=None, gt=None):
        """r: the expected first words of the result slot; flag; gt: twelve integers, the expected GT words"""
        assert len(x0) <= 108 and len(x1) <= 108
        self.rows.append((OPS.index(op), flags, list(x0), list(x1), r, flag, gt))

    def write(self, path):
        self.rows.sort(key=lambda t: t[0])
        a = np.zeros((len(self.rows), CASE_WORDS), dtype=np.uint32)
        for i, (op, flags, x0, x1, *_) in enumerate(self.rows):
            a[i, 0], a[i, 1] = op, flags
            a[i, 2:2 + len(x0)] = x0
            a[i, 110:110 + len(x1)] = x1
        a.tofile(path)
        counts = {}
        for row in self.rows:
            counts[OPS[row[0]]] = counts.get(OPS[row[0]], 0) + 1
        return counts

    def judge(self, path):
        got = np.fromfile(path, dtype=np.uint32)
        assert got.size == len(self.rows) * OUT_WORDS
        got = got.reshape(-1, OUT_WORDS).tolist()
        bad, first = [], {}
        for i, (op, flags, x0, x1, r, flag, gt) in enumerate(self.rows):
            first.setdefault(op, i)
            o, why = got[i], None
            if r is not None and o[:len(r)] != r:
                why = "result words differ"
            if flag is not None and o[108] != flag:
                why = "flag %d, expected %d" % (o[108], flag)
            if gt is not None and [unwords(o[109 + 8 * k:117 + 8 * k]) for k in range(12)] != gt:
                why = "GT words differ"
            if why:
                bad.append((OPS[op], i - first[op], why))
        return bad


def make_cases():
    C = Cases()
    rng = random.Random(0x9A121)
    ops = fq_operands()
    rnd12 = lambda: [rng.randrange(Q) for _ in range(12)]
    # the inverses: Fermat, 0 -> 0
    for v in ops[:48]:
        C.add("fq_inv", mont(v), r=mont(pow(v, Q - 2, Q)))
    for a in [(0, 0), (1, 0), (0, 1), (Q - 1, Q - 1), (ops[9], 0), (0, ops[11])] + [(rng.choice(ops), rng.randrange(Q)) for _ in range(16)]:
        C.add("fq2_inv", mont(a[0]) + mont(a[1]), r=(mont(0) * 2 if a == (0, 0) else [x for c in B.f2_inv(a) for x in mont(c)]))
    # F_q12 elements whose coefficients are corners, and random ones
    corner12 = [[0] * 12, BP.ONE, [Q - 1] * 12, [1] * 12, [0] * 11 + [Q - 1]] + [[rng.choice(ops) for _ in range(12)] for _ in range(6)]
    elems = corner12 + [rnd12() for _ in range(5)]
    for a in elems:
        b = rng.choice(elems)
        C.add("fq12_mul", flat_limbs(a), flat_limbs(b), r=flat_limbs(BP.f_mul(a, b)))
        C.add("fq12_sqr", flat_limbs(a), r=flat_limbs(BP.f_mul(a, a)))
        l = [(rng.choice(ops), rng.choice(ops)) for _ in range(3)]          # l0 + l1 w + l3 w^3 with F_q2 coefficients
        line = [0] * 12
        for pos, (c0, c1) in zip((0, 1, 3), l):
            line[pos], line[pos + 6] = (c0 - 9 * c1) % Q, c1
        C.add("fq12_mul_line", flat_limbs(a), [x for c in l for x in mont(c[0]) + mont(c[1])], r=flat_limbs(BP.f_mul(a, line)))
    for a in elems[1:]:
        if a != [1] * 12:
            inv = BP.f_inv(a)
            assert BP.f_mul(a, inv) == BP.ONE
            C.add("fq12_inv", flat_limbs(a), r=flat_limbs(inv))
    C.add("fq12_inv", flat_limbs([0] * 12), r=flat_limbs([0] * 12))          # through the Fermat inverse: 0
    for a in [elems[0], elems[1], elems[2], elems[5], elems[-1]]:
        C.add("fq12_conj", flat_limbs(a), r=flat_limbs(BP.f_pow(a, Q ** 6)))
        for k in (1, 2, 3):
            C.add("fq12_frob%d" % k, flat_limbs(a), r=flat_limbs(BP.f_pow(a, Q ** k)))
    # the final exponentiation alone: random elements are outside every subgroup, so a multiple of the exponent shows
    for a in [[0] * 12, BP.ONE, elems[2], rnd12(), rnd12()]:
        want = BP.final_exp(a)
        C.add("fq12_final_exp", flat_limbs(a), r=flat_limbs(want), gt=want)
    # whole pairings
    off = off_subgroup_point()
    g1s, g2s = ref_vk_points()
    for _ in range(3):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        P, Q2 = B.mul(B.G, a), B.mul_g2(B.G2, b)
        C.add("pairing", g1_words(P) + g2_words(Q2), flag=0, gt=BP.pairing(Q2, P))
    C.add("pairing", g1_words(g1s[0]) + g2_words(g2s[0]), flag=0, gt=BP.pairing(g2s[0], g1s[0]))
    for a, b in [(1, 1), (2, 3), (5, 1), (R - 1, 1), (1, R - 1), (7, 11)] + [(rng.randrange(1, 1 << 16), rng.randrange(1, 1 << 16)) for _ in range(10)]:
        C.add("pairing", g1_words(B.mul(B.G, a)) + g2_words(B.mul_g2(B.G2, b)), flag=0, gt=BP.f_pow(e1(), a * b % R))
    C.add("pairing", g1_words(None) + g2_words(B.G2), flag=0, gt=BP.ONE)
    C.add("pairing", g1_words(B.G) + g2_words(None), flag=0, gt=BP.ONE)
    C.add("pairing", words(Q) + words(2) + g2_words(B.G2), flag=1)
    C.add("pairing", g1_words(B.G) + words(1) + words(Q) + words(0) * 2, flag=1)
    C.add("pairing", g1_words((1, 3)) + g2_words(B.G2), flag=2)
    C.add("pairing", g1_words(B.G) + g2_words(((1, 2), (3, 4))), flag=2)
    C.add("pairing", g1_words(B.G) + g2_words(off), flag=3)
    C.add("pairing", g1_words(B.G) + g2_words(off), flags=1, flag=0)          # the subgroup test skipped (a key's point): no refusal
    # the G2 checks: bit 0 on the twist, bit 1 [r]Q = O
    for p in [B.mul_g2(B.G2, k) for k in (1, 2, 3, R - 1, rng.randrange(R))] + g2s + [off, B.mul_g2(off, 5)]:
        C.add("g2_checks", g2_words(p), flag=(1 if B.on_curve_g2(p) else 0) | (2 if B.mul_g2(p, R) is None else 0))
    return C


_MADE = {}


def run_and_judge(exe, d):
    if "c" not in _MADE:
        _MADE["c"] = make_cases()
    C = _MADE["c"]
    cases, results = os.path.join(d, "p12_cases.bin"), os.path.join(d, "p12_results.bin")
    counts = C.write(cases)
    out = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    seen = {m[1]: int(m[2]) for m in re.finditer(r"^prim (\S+) cases (\d+)$", out.stdout, re.M)}
    assert sorted(seen) == sorted(OPS)
    for op in OPS:
        assert seen[op] == counts.get(op, 0) > 0, (op, seen[op], counts.get(op, 0))
    print("cases per operation:", counts)
    return C.judge(results), out.stdout


def build_host(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-I", CSRC, SRC, "-o", exe])


@pytest.mark.parametrize("build", ["plain", "san"])
def test_pairing254_host(tmp_path, build):
    exe = str(tmp_path / "pairing254_check_host")
    build_host(exe, extra=SAN if build == "san" else ())
    bad, out = run_and_judge(exe, str(tmp_path))
    assert "build host" in out
    assert not bad, "%d complaints, the first: %s" % (len(bad), bad[:8])


def test_constants_file_is_what_its_generator_writes():
    import sys
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_pairing254_constants.py"), "--check"])

