"""The BN254 base field and the curve code under every MSM (csrc/fq254.hpp) at the bounds its comments state: F_q and F_q2 on nine 29-bit limbs
(R = 2^261 ~ 169.28 q), the lazy unreduced forms of the G1 bucket sums, the Jacobian formulas over both fields.

tests/native/fq254_check.hip runs every function on a case file and writes every word each one returns; it judges nothing.  The cases and all
expectations are made here with Python integers and oracle/naive_bn254.py:  fq_mul(a, b) is a b / R mod q whatever a and b stand for, lz_mul is
the exact integer (a b + m q) / R, and jac_madd_lazy is modelled step by step on integers, so its raw result is compared word for word and every
bound of its comment (each lz_sub non-negative, each product below 169 q^2, the accumulator invariant) is checked on the way.

Host builds run anywhere (g++, also under UBSan+ASan: stand-alone programs) and cover the lazy forms too, whose bodies are plain C++.  The device
program is built with hipcc for gfx950 and runs one case per lane as a fresh child process."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import naive_bn254 as B
from test_field_corners import ARCH, CSRC, HIPCC, NATIVE, run_latched

Q = B.Q
RR = 1 << 261                        # the Montgomery radix
RINV = pow(RR, -1, Q)
QINV = pow(Q, -1, RR)
MASK29 = (1 << 29) - 1
ONE = RR % Q                         # fq_one()
SAN = ("-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")

OPS = ["fq_add", "fq_sub", "fq_dbl", "fq_mul", "fq_sqr", "fq_to_mont", "fq_from_mont", "fq_mont_round_trip", "fq_from_words", "fq_words_round_trip",
       "fq_is_zero_eq", "fq_norm_sub", "fq_neg_lazy", "fq_mul2", "f2_mul", "f2_sqr", "f2_add", "f2_sub", "f2_dbl", "fq_inv_host", "f2_inv_host",
       "lz_mul", "lz_sub<1>", "lz_sub<3>", "lz_sub<5>", "lz_sub<6>", "lz_sub<7>", "lz_sub2<4>", "lz_add", "lz_dbl", "lz_quad", "lz_canon", "lz_is_zero_mod_q",
       "g1_jac_dbl", "g1_jac_madd", "g1_jac_add", "g1_jac_mul_small", "g2_jac_dbl", "g2_jac_madd", "g2_jac_add", "g2_jac_mul_small",
       "jac_madd_lazy", "jac_madd_lazy_chain"]
HOST_ONLY = ("fq_inv_host", "f2_inv_host")
CASE_WORDS, OUT_WORDS = 118, 90      # u32 op, k, x[12][9], w[8]  /  u32 r[9][9], flag, w[8]


# ---------------------------------------------------------------------------------------------------------------- limb forms
def limbs(v):
    """normalised: nine limbs below 2^29"""
    assert 0 <= v < RR, v
    return [(v >> (29 * i)) & MASK29 for i in range(9)]


def nform(v):
    """the N form of the lazy code: limbs 0..7 below 2^29, the top limb holds the rest"""
    assert 0 <= v < 1 << (232 + 32), v
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def denorm(l, i, k=1):
    """the same value with k 2^29 moved from limb i + 1 down into limb i"""
    l = list(l)
    assert 0 <= i < 8 and l[i + 1] >= k
    l[i] += k << 29
    l[i + 1] -= k
    return l


def doubled(v):
    """v as lz_dbl leaves it: every limb twice the limb of v / 2 (an odd v keeps its last bit in limb 0)"""
    return [2 * x + (v & 1 if i == 0 else 0) for i, x in enumerate(nform(v >> 1))]


def words(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def all_ones_below_q():
    v = (((Q >> 232) - 1) << 232) | ((1 << 232) - 1)
    assert v < Q and all(l == MASK29 for l in limbs(v)[:8])
    return v


def fq_operands():
    vals = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, ONE, RR * RR % Q]
    for k in (28, 29, 30, 58, 87, 232, 253):
        vals += [1 << k, (1 << k) - 1]
    vals.append(all_ones_below_q())
    # q's own limbs with one of them a unit off, as far as the value stays below q: limb i less one; limb i plus one under limb i + 1 less one
    vals += [Q - (1 << (29 * i)) for i in range(9)] + [Q + (1 << (29 * i)) - (1 << (29 * (i + 1))) for i in range(8)]
    rng = random.Random(0xF9254)
    vals += [rng.randrange(Q) for _ in range(64)]
    assert all(0 <= v < Q for v in vals) and len(vals) == 40 + 64
    return vals


def lzmul(a, b):
    """lz_mul on integers: (a b + m q) / R with m = -a b / q mod R; its contract a b < 169 q^2 and its return bound are asserted"""
    assert a * b < 169 * Q * Q, "product outside 169 q^2: %.3f" % (a * b / (Q * Q))
    m = (-a * b * QINV) % RR
    r, rem = divmod(a * b + m * Q, RR)
    assert rem == 0 and 169 * Q * r < 169 * Q * Q + a * b          # r < (1 + a b / 169 q^2) q
    return r


# ---------------------------------------------------------------------------------------------------------------- the case list
class Cases:
    def __init__(self):
        self.rows = []

    def add(self, op, xs=(), k=0, w=None, exp=None, flag=None, wexp=None, fn=None):
        """xs: limb lists as the function takes them; exp: {slot: limbs} compared word for word; fn(out words) -> a complaint or None"""
        assert len(xs) <= 12 and all(len(x) == 9 and all(0 <= v < 1 << 32 for v in x) for x in xs)
        self.rows.append((OPS.index(op), k, xs, w, exp or {}, flag, wexp, fn))

    def write(self, path):
        self.rows.sort(key=lambda t: t[0])       # the program wants the cases of an operation together (stable: the order within stays)
        flat = []
        for op, k, xs, w, *_ in self.rows:
            row = [op, k]
            for x in xs:
                row += x
            row += [0] * (2 + 108 - len(row)) + (w or [0] * 8)
            flat.append(row)
        a = np.array(flat, dtype=np.uint32)
        assert a.shape == (len(self.rows), CASE_WORDS)
        a.tofile(path)
        counts = {}
        for r in self.rows:
            counts[OPS[r[0]]] = counts.get(OPS[r[0]], 0) + 1
        return counts

    def judge(self, path):
        """-> the complaints, (operation, case number within it, what)"""
        got = np.fromfile(path, dtype=np.uint32)
        assert got.size == len(self.rows) * OUT_WORDS, (got.size, len(self.rows))
        got = got.reshape(-1, OUT_WORDS).tolist()
        bad, first = [], {}
        for i, (op, k, xs, w, exp, flag, wexp, fn) in enumerate(self.rows):
            first.setdefault(op, i)
            o = got[i]
            why = None
            for slot, e in exp.items():
                if o[9 * slot:9 * slot + 9] != e:
                    why = "slot %d: got %s want %s" % (slot, [hex(v) for v in o[9 * slot:9 * slot + 9]], [hex(v) for v in e])
            if flag is not None and o[81] != flag:
                why = "flag %d want %d" % (o[81], flag)
            if wexp is not None and o[82:90] != wexp:
                why = "words differ"
            if why is None and fn is not None:
                try:
                    why = fn(o)
                except AssertionError as e:
                    why = "assert " + str(e)
            if why:
                bad.append((OPS[op], i - first[op], why))
        return bad


def slot(o, j):
    return o[9 * j:9 * j + 9]


def field_cases(C, host):
    vals = fq_operands()
    L = {v: limbs(v) for v in vals}
    for a in vals:
        for b in vals:
            C.add("fq_add", (L[a], L[b]), exp={0: limbs((a + b) % Q)})
            C.add("fq_sub", (L[a], L[b]), exp={0: limbs((a - b) % Q)})
            C.add("fq_mul", (L[a], L[b]), exp={0: limbs(a * b * RINV % Q)})
            C.add("fq_is_zero_eq", (L[a], L[b]), flag=int(a == 0) | 2 * int(a == b))
        C.add("fq_dbl", (L[a],), exp={0: limbs(2 * a % Q)})
        C.add("fq_sqr", (L[a],), exp={0: limbs(a * a * RINV % Q)})
        C.add("fq_to_mont", (L[a],), exp={0: limbs(a * RR % Q)})
        C.add("fq_from_mont", (L[a],), exp={0: limbs(a * RINV % Q)})
        C.add("fq_mont_round_trip", (L[a],), exp={0: L[a]})
        C.add("fq_words_round_trip", (L[a],), exp={0: L[a]}, wexp=words(a))
        C.add("fq_neg_lazy", (L[a],), exp={0: limbs(Q - a)})          # in (0, q], congruent to -a, normalised: q itself for a = 0
        C.add("fq_from_words", w=words(a), exp={0: L[a]}, wexp=words(a))
        if host and a:
            C.add("fq_inv_host", (L[a],), exp={0: limbs(RR * RR * pow(a, -1, Q) % Q)})          # Montgomery form in and out: a r / R = R
    for w in (Q, Q + 1, 1 << 255, (1 << 256) - 1):
        C.add("fq_from_words", w=words(w), exp={0: limbs(w)}, wexp=words(w))       # the slices of whatever 256 bits it is given
    # fq_norm_sub at its stated domain: limbs below 2^31, value below 2 q
    rng = random.Random(0x5B)
    for v in [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, Q + all_ones_below_q(), 2 * all_ones_below_q()] + [rng.randrange(2 * Q) for _ in range(32)]:
        forms = [limbs(v)]
        for i in range(8):
            for k in (1, 2, 3):
                if forms[0][i + 1] >= k:
                    forms.append(denorm(forms[0], i, k))                   # limb i up to 2^31 - 1
        if v <= 2 * Q - 2:                                                 # the limbwise sum of two canonical values, as fq_add forms it
            a = rng.randrange(max(v - Q + 1, 0), min(v, Q - 1) + 1)
            forms.append([x + y for x, y in zip(limbs(a), limbs(v - a))])
        for t in forms:
            assert val(t) == v < 2 * Q and max(t) < 1 << 31
            C.add("fq_norm_sub", (t,), exp={0: limbs(v % Q)})
    # fq_mul2: limbs below 2^29, one operand of each product below 2^30, a b + c d below 169 q^2
    top = all_ones_below_q()
    full = RR - 1                                                          # all nine limbs ones: 169.28 q
    quads = [(L[Q - 1],) * 4, (L[top], doubled(2 * top), L[top], doubled(2 * top)), (L[Q - 1], doubled(2 * (Q - 1)), L[Q - 2], doubled(2 * top)),
             (doubled(2 * top), L[top], doubled(2 * top), L[Q - 1])]
    assert max(doubled(2 * top)[:8]) == min(doubled(2 * top)[:8]) == (1 << 30) - 2
    b = (169 * Q * Q - 1) // (2 * full)
    d = (169 * Q * Q - 1 - full * b) // full
    assert 169 * Q * Q - full <= full * b + full * d < 169 * Q * Q
    quads += [(limbs(full), limbs(b), limbs(full), limbs(d)), (limbs(b), limbs(full), limbs(d), limbs(full))]
    b = (169 * Q * Q - 1) // (13 * Q)                                      # with the second operand of each product in doubled form
    quads += [(limbs(13 * Q // 2), doubled(b), limbs(13 * Q // 2), doubled(b - 1))]
    for _ in range(256):
        quads.append(tuple(L[rng.choice(vals)] if rng.random() < 0.3 else limbs(rng.randrange(Q)) for _ in range(4)))
    for _ in range(64):                                                    # as f_mul and f_sqr call it: (a0, b0, q - a1, b1), a doubled operand
        a0, a1, b0 = (rng.choice(vals) for _ in range(3))
        quads.append((L[a0], doubled(2 * b0), limbs(Q - a1), doubled(2 * a1)))
    for q4 in quads:
        a_, b_, c_, d_ = (val(x) for x in q4)
        assert a_ * b_ + c_ * d_ < 169 * Q * Q and all(max(x) < 1 << 30 for x in q4)
        assert max(q4[0]) <= MASK29 or max(q4[1]) <= MASK29
        assert max(q4[2]) <= MASK29 or max(q4[3]) <= MASK29
        C.add("fq_mul2", q4, exp={0: limbs((a_ * b_ + c_ * d_) * RINV % Q)})
    # F_q2
    xs = [1, 2, Q - 1, Q - 2, (Q - 1) // 2, top, ONE] + [rng.randrange(Q) for _ in range(8)]
    pairs = [((0, x), (0, x)) for x in xs] + [((x, 0), (x, 0)) for x in xs] + [((0, x), (x, 0)) for x in xs]
    pairs += [((Q - 1, Q - 1), (Q - 1, Q - 1))] + [((x, x), (x, x)) for x in xs] + [((x, Q - x), (x, Q - x)) for x in xs]
    pairs += [((x, x), (y, Q - y)) for x in xs[:4] for y in xs[:4]]
    pairs += [((rng.randrange(Q), rng.randrange(Q)), (rng.randrange(Q), rng.randrange(Q))) for _ in range(64)]
    pairs += [((rng.choice(vals), rng.choice(vals)), (rng.choice(vals), rng.choice(vals))) for _ in range(64)]

    def f2l(a):
        return {0: limbs(a[0]), 1: limbs(a[1])}

    def scale(a, s):
        return (a[0] * s % Q, a[1] * s % Q)
    for a, b in pairs:
        ops = (limbs(a[0]), limbs(a[1]), limbs(b[0]), limbs(b[1]))
        C.add("f2_mul", ops, exp=f2l(scale(B.f2_mul(a, b), RINV)))
        C.add("f2_sqr", ops[:2], exp=f2l(scale(B.f2_mul(a, a), RINV)))
        C.add("f2_add", ops, exp=f2l(B.f2_add(a, b)))
        C.add("f2_sub", ops, exp=f2l(B.f2_sub(a, b)))
        C.add("f2_dbl", ops[:2], exp=f2l(B.f2_add(a, a)))
        if host and a != (0, 0):
            C.add("f2_inv_host", ops[:2], exp=f2l(scale(B.f2_inv(a), RR * RR % Q)))


def lazy_cases(C):
    rng = random.Random(0x1A2)
    vals = fq_operands()
    full = RR - 1
    # ---- lz_mul: limbs below 2^30 in both operands, a b below 169 q^2
    pairs = [(nform(13 * Q - 1), nform(13 * Q)), (nform(13 * Q), nform(13 * Q - 1)), (limbs(full), limbs((169 * Q * Q - 1) // full)),
             (nform(169 * Q - 1), nform(Q)), (nform(Q), nform(169 * Q - 1)), (nform(0), nform(169 * Q - 1)), (nform(1), nform(1))]
    for v in (12 * Q - 2, 12 * Q - 1, 12 * Q - 3, 8 * Q - 1, 2 * Q - 1):          # rr = 2 r0 < 12.03 q as lz_dbl leaves it, squared
        pairs.append((doubled(v), doubled(v)))
    for v, u in [(13 * Q - 1, 13 * Q), (7 * Q - 1, 5 * Q + 12345), (2 * Q - 1, 2 * Q - 1), (Q + all_ones_below_q(), 8 * Q)]:
        for i in range(8):                      # denormalised forms of one value: limb i up by 2^29 under limb i + 1 down by one, in either operand or both
            if nform(v)[i + 1] and nform(u)[i + 1]:
                pairs += [(denorm(nform(v), i), nform(u)), (nform(v), denorm(nform(u), i)), (denorm(nform(v), i), denorm(nform(u), i))]
    both = nform(13 * Q - 1)                    # every other limb at 2^30 - 1 or close
    for i in (0, 2, 4, 6):
        both = denorm(both, i)
    pairs.append((both, both))
    pairs += [(limbs(a), limbs(b)) for a in vals[:41:3] for b in vals[:41:3]]
    for _ in range(128):
        a = rng.randrange(13 * Q)
        pairs.append((doubled(a), nform(rng.randrange(min(13 * Q, 169 * Q * Q // (a + 1))))))
    for a, b in pairs:
        assert max(a) < 1 << 30 and max(b) < 1 << 30
        r = lzmul(val(a), val(b))
        C.add("lz_mul", (a, b), exp={0: nform(r)})
    # ---- lz_sub<K>(a, b) = a - b + K q in N form, K q >= b;  lz_sub2<4>(a, b, d) = a - b - d + 4 q
    for K in (1, 3, 5, 6, 7):
        cases = [(0, nform(K * Q)), (0, nform(K * Q - 1)), (0, nform(0)), (Q - 1, nform(0)), (2 * Q - 1, nform(0)), (7 * Q - 1, nform(0)),
                 (2 * Q - 1, nform(K * Q)), (1, nform(K * Q)), (Q - 1, nform(K * Q - 1))]
        cases += [(rng.randrange(2 * Q), nform(K * Q)) for _ in range(4)] + [(rng.randrange(2 * Q), nform(rng.randrange(K * Q + 1))) for _ in range(16)]
        if K > 1:
            cases += [(0, doubled(K * Q)), (0, doubled(K * Q - 1)), (rng.randrange(2 * Q), doubled(K * Q))]      # b as lz_dbl leaves it
        for i in range(8):
            cases.append((0, denorm(nform(K * Q), i)))
        for a, b in cases:
            C.add("lz_sub<%d>" % K, (nform(a), b), exp={0: nform(a - val(b) + K * Q)})
    cases = [(0, 4 * Q, 0), (0, 0, 4 * Q), (0, 2 * Q, 2 * Q), (0, 2 * Q - 1, 2 * Q), (0, 2 * Q, 2 * Q - 1), (0, 0, 0), (2 * Q - 1, 0, 0), (2 * Q - 1, 2 * Q - 1, 2 * Q),
             (1, 4 * Q, 0), (0, Q + 1, 3 * Q - 1)]
    cases += [(rng.randrange(2 * Q), b, 4 * Q - b) for b in (rng.randrange(2 * Q) for _ in range(8))]
    cases += [(rng.randrange(2 * Q), rng.randrange(2 * Q), rng.randrange(2 * Q)) for _ in range(16)]
    for a, b, d in cases:
        C.add("lz_sub2<4>", (nform(a), nform(b), doubled(d)), exp={0: nform(a - b - d + 4 * Q)})          # d = 2 V comes from lz_dbl
        C.add("lz_sub2<4>", (nform(a), nform(b), nform(d)), exp={0: nform(a - b - d + 4 * Q)})
    # ---- limbwise forms
    ns = [0, 1, Q - 1, Q, 2 * Q - 1, 7 * Q - 1, RR - 1, all_ones_below_q() + Q] + [rng.randrange(7 * Q) for _ in range(16)]
    for a in ns:
        for b in ns[:8]:
            C.add("lz_add", (nform(a), nform(b)), exp={0: [x + y for x, y in zip(nform(a), nform(b))]})
        C.add("lz_dbl", (nform(a),), exp={0: [2 * x for x in nform(a)]})
        C.add("lz_quad", (nform(a),), exp={0: nform(4 * a)})
    # ---- lz_canon: values up to 169 q - 1 on limbs below 2^30
    cs = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q, 7 * Q - 1, 169 * Q - 1, 169 * Q - 2, 168 * Q, 168 * Q + 1] + [rng.randrange(169 * Q) for _ in range(32)]
    for v in cs:
        forms = [limbs(v), doubled(v)] + [denorm(limbs(v), i) for i in range(8) if limbs(v)[i + 1]]
        for t in forms:
            assert val(t) == v and max(t) < 1 << 30
            C.add("lz_canon", (t,), exp={0: limbs(v % Q)})
    for v in (0, Q, Q + 1, Q - 1, 2 * Q - 1, 1, Q - (1 << 232), Q ^ (1 << 116)):
        C.add("lz_is_zero_mod_q", (nform(v),), flag=int(v % Q == 0))


# ---------------------------------------------------------------------------------------------------------------- curve
def mont(v):
    return limbs(v * RR % Q)


class G1:
    name, n = "g1", 1
    add, mul, gen = staticmethod(B.add), staticmethod(B.mul), B.G

    @staticmethod
    def neg(p):
        return (p[0], (-p[1]) % Q)

    @staticmethod
    def jac(p, z):
        """the limbs of p under Z = z, Montgomery form"""
        if p is None:
            return [mont(z), mont(z * z % Q + 1), limbs(0)]          # any X, Y over Z = 0
        return [mont(p[0] * z * z % Q), mont(p[1] * z * z * z % Q), mont(z)]

    @staticmethod
    def aff(p):
        return [mont(p[0]), mont(p[1])]

    @staticmethod
    def affine_of(ls, canonical=True):
        """raw Jacobian limbs (three elements) -> the affine point, or None for Z = 0 exactly"""
        if canonical:
            assert all(l == limbs(val(l) % Q) for l in ls), "not fully reduced"
        X, Y, Z = (val(l) * RINV % Q for l in ls)
        if not any(ls[2]):
            return None
        assert Z, "Z is a multiple of q but not the exact zero"
        zi = pow(Z, -1, Q)
        return (X * zi * zi % Q, Y * zi * zi * zi % Q)

    @staticmethod
    def rand_z(rng):
        return rng.randrange(1, Q)


class G2:
    name, n = "g2", 2
    add, mul, gen = staticmethod(B.add_g2), staticmethod(B.mul_g2), B.G2

    @staticmethod
    def neg(p):
        return (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))

    @staticmethod
    def _m2(a):
        return [mont(a[0]), mont(a[1])]

    @staticmethod
    def jac(p, z):
        if p is None:
            return G2._m2(z) + G2._m2(B.f2_mul(z, z)) + [limbs(0), limbs(0)]
        z2 = B.f2_mul(z, z)
        return G2._m2(B.f2_mul(p[0], z2)) + G2._m2(B.f2_mul(p[1], B.f2_mul(z2, z))) + G2._m2(z)

    @staticmethod
    def aff(p):
        return G2._m2(p[0]) + G2._m2(p[1])

    @staticmethod
    def affine_of(ls, canonical=True):
        assert all(l == limbs(val(l) % Q) for l in ls), "not fully reduced"
        X, Y, Z = (((val(ls[2 * j]) * RINV) % Q, (val(ls[2 * j + 1]) * RINV) % Q) for j in range(3))
        if not any(ls[4]) and not any(ls[5]):
            return None
        zi = B.f2_inv(Z)
        zi2 = B.f2_mul(zi, zi)
        return (B.f2_mul(X, zi2), B.f2_mul(Y, B.f2_mul(zi2, zi)))

    @staticmethod
    def rand_z(rng):
        return (rng.randrange(Q), rng.randrange(1, Q))


def curve_cases(C):
    for grp in (G1, G2):
        rng = random.Random(0xC0 + grp.n)
        T = [grp.mul(grp.gen, k) for k in [1, 2, 3, 5, 7, 11] + [rng.randrange(1, B.R) for _ in range(6)]]
        one = (1, 0) if grp is G2 else 1
        nel = 3 * grp.n

        def want(p):
            def fn(o, p=p, grp=grp, nel=nel):
                got = grp.affine_of([slot(o, j) for j in range(nel)])
                return None if got == p else "point %s want %s" % (got, p)
            return fn

        def zs():
            return (one, grp.rand_z(rng))
        for p in T:
            for z in zs():
                C.add(grp.name + "_jac_dbl", grp.jac(p, z), fn=want(grp.add(p, p)))
                for k in (0, 1, 2, 3, 1 << 16, (1 << 32) - 1):
                    C.add(grp.name + "_jac_mul_small", grp.jac(p, z), k=k, fn=want(grp.mul(p, k)))
        for z in zs():
            C.add(grp.name + "_jac_dbl", grp.jac(None, z), fn=want(None))
            C.add(grp.name + "_jac_mul_small", grp.jac(None, z), k=5, fn=want(None))
            C.add(grp.name + "_jac_add", grp.jac(None, z) + grp.jac(None, one), fn=want(None))
        for i, p in enumerate(T):
            q = T[(i + 5) % len(T)]
            for z in zs():
                z2 = grp.rand_z(rng)
                for a, b in ((p, q), (p, p), (p, grp.neg(p)), (None, p), (p, None)):
                    C.add(grp.name + "_jac_add", grp.jac(a, z) + grp.jac(b, z2), fn=want(grp.add(a, b)))        # (p, p): one point under two Z
                C.add(grp.name + "_jac_add", grp.jac(p, z) + grp.jac(p, z), fn=want(grp.add(p, p)))
                for a, b in ((p, q), (p, p), (p, grp.neg(p)), (None, p)):
                    C.add(grp.name + "_jac_madd", grp.jac(a, z) + grp.aff(b), fn=want(grp.add(a, b)))


# ---------------------------------------------------------------------------------------------------------------- jac_madd_lazy
class LazyStats:
    def __init__(self):
        self.max = {k: 0 for k in ("X3", "Y3", "Z3", "H", "rr")}
        self.branch = {"doubling": 0, "infinity": 0, "accumulator at infinity": 0, "general": 0}
        self.tight = {"lz_sub<7>": 0, "lz_sub<5>": 0, "lz_sub2<4>": 0}      # cases in which one q less would have gone negative

    def see(self, **kw):
        for k, v in kw.items():
            self.max[k] = max(self.max[k], v)


def madd_lazy_model(X, Y, Z, qx, qy, stats):
    """jac_madd_lazy step by step on integers (values of the raw limbs): -> (X3, Y3, Z3) or None where it hands over to the canonical code.
    Every lz_sub is asserted non-negative and lzmul asserts every product below 169 q^2."""
    Z1Z1 = lzmul(Z, Z)
    U2 = lzmul(qx, Z1Z1)
    S2 = lzmul(lzmul(qy, Z), Z1Z1)
    H = U2 - X + 7 * Q
    assert H >= 0
    HH = lzmul(H, H)
    if HH % Q == 0:
        assert HH in (0, Q)
        return None
    I = 4 * HH
    J = lzmul(H, I)
    r0 = S2 - Y + 5 * Q
    assert r0 >= 0
    rr = 2 * r0
    V = lzmul(X, I)
    rr2 = lzmul(rr, rr)
    X3 = rr2 - J - 2 * V + 4 * Q
    assert X3 >= 0
    t = V - X3 + 6 * Q
    assert t >= 0
    Y3 = lzmul(rr, t) - 2 * lzmul(Y, J) + 3 * Q
    assert Y3 >= 0
    Z3 = 2 * lzmul(Z, H)
    stats.see(X3=X3, Y3=Y3, Z3=Z3, H=H, rr=rr)
    stats.tight["lz_sub<7>"] += U2 - X + 6 * Q < 0
    stats.tight["lz_sub<5>"] += S2 - Y + 4 * Q < 0
    stats.tight["lz_sub2<4>"] += rr2 - J - 2 * V + 3 * Q < 0
    return X3, Y3, Z3


def check_invariant(ls):
    """the accumulator invariant of jac_madd_lazy's comment on raw limbs: X in N(7), Y in N(5), Z in W(2.3)"""
    X, Y, Z = (val(l) for l in ls)
    assert X < 7 * Q and Y < 5 * Q and 10 * Z < 23 * Q, "outside the invariant: %.3f %.3f %.3f" % (X / Q, Y / Q, Z / Q)
    assert max(ls[0][:8]) <= MASK29 and max(ls[1][:8]) <= MASK29 and max(ls[2]) < 1 << 30, "limbs outside the invariant"


def lazy_judge(acc_limbs, qx, qy_eff, want_pt, stats, model=True):
    """-> fn(out words) for one jac_madd_lazy case; the branch is counted when the case is made"""
    X, Y, Z = (val(l) for l in acc_limbs)
    if not any(acc_limbs[2]):
        exp, kind = (limbs(qx), nform(qy_eff), limbs(ONE)), "accumulator at infinity"
    else:
        m = madd_lazy_model(X, Y, Z, qx, qy_eff, stats)
        if m is None:
            exp, kind = None, "infinity" if want_pt is None else "doubling"
        else:
            exp, kind = (nform(m[0]), nform(m[1]), [2 * x for x in nform(m[2] // 2)]), "general"
    stats.branch[kind] += 1

    def fn(o):
        raw = [slot(o, j) for j in range(3)]
        if exp is not None and model:
            assert tuple(raw) == tuple(exp), "raw result differs from the integer model"
        check_invariant(raw)
        got = G1.affine_of(raw, canonical=False)
        assert got == want_pt, "point %s want %s" % (got, want_pt)
        if want_pt is None:
            assert not any(raw[2])
        for j in range(3):
            assert slot(o, 3 + j) == limbs(val(raw[j]) % Q), "jac_canon is not fully reduced"
        return None
    return fn, kind


def z_reps(vmax, t):
    """every representative of Z the invariant allows, given the largest one (vmax < 2.3 q, limb t at 2^29 - 2): (value, limbs)"""
    reps = []
    v = vmax
    while v >= 0:
        n = nform(v)
        forms = [n, doubled(v)] + [denorm(n, i) for i in (t, (t + 3) % 8) if n[i + 1]]
        reps += [(v, f) for f in forms]
        v -= Q
    assert reps[2][1][t] == (1 << 30) - 2          # the largest Z with limb t as high as a doubled limb goes
    return reps


def madd_lazy_cases(C, stats):
    rng = random.Random(0xD1)
    T = [B.mul(B.G, rng.randrange(1, B.R)) for _ in range(12)]
    npairs = 0

    def one(acc_pt, z, kx, ky, zl, p, neg):
        """the accumulator acc_pt under Z = z, written as X + kx q, Y + ky q and the limbs zl of some Z + k q"""
        X = acc_pt[0] * z * z % Q * RR % Q + kx * Q
        Y = acc_pt[1] * z * z * z % Q * RR % Q + ky * Q
        acc = [nform(X), nform(Y), zl]
        qx, qy = p[0] * RR % Q, p[1] * RR % Q
        eff = G1.neg(p) if neg else p
        fn, kind = lazy_judge(acc, qx, Q - qy if neg else qy, B.add(acc_pt, eff), stats)
        C.add("jac_madd_lazy", acc + [limbs(qx), limbs(qy)], k=neg, fn=fn)
        return kind

    for n in range(64):
        a, p, neg = T[n % 12], T[(n // 12 + 1 + n) % 12], n & 1
        assert a != p
        for big in (0, 1):
            # the largest representative first: below 2.3 q (Z + 2 q) or below 2 q (Z + q), limb t at 2^29 - 2; Z itself is what is left
            t = rng.randrange(7)
            vmax = rng.randrange(22 * Q // 10, 23 * Q // 10) if big else rng.randrange(Q + 1, 2 * Q)
            vmax = (vmax & ~(MASK29 << (29 * t))) | (((1 << 29) - 2) << (29 * t))
            if nform(vmax)[t + 1] == 0:
                vmax += 1 << (29 * (t + 1))
            assert 10 * vmax < 23 * Q
            reps = z_reps(vmax, t)
            z = vmax % Q * RINV % Q
            todo = set()
            for zi in range(len(reps)):
                todo |= {(6, 4, zi), (0, 0, zi), (6, 0, zi), (0, 4, zi)}
            for kx in range(7):
                for ky in range(5):
                    todo.add((kx, ky, rng.randrange(len(reps))))
            for kx, ky, zi in sorted(todo):
                assert one(a, z, kx, ky, reps[zi][1], p, neg) == "general"
        npairs += 1
    # cases picked with the model so that each lz_sub of the general path is met where one q less would go negative (what a wrong K changes)
    want_tight = 24
    for _ in range(40000):
        if stats.tight["lz_sub2<4>"] >= want_tight:
            break
        a, p = rng.sample(T, 2)
        zv = rng.randrange(1, Q)
        X, Y = a[0] * zv * zv % Q * RR % Q, a[1] * zv ** 3 % Q * RR % Q
        probe = LazyStats()
        madd_lazy_model(X, Y, zv * RR % Q, p[0] * RR % Q, p[1] * RR % Q, probe)
        if probe.tight["lz_sub2<4>"]:
            one(a, zv, 0, 0, nform(zv * RR % Q), p, 0)
    # the canonical fallback: the accumulator is +-the point (in a non-zero representative) or infinity
    for n in range(12):
        p, neg = T[n], n & 1
        eff = G1.neg(p) if neg else p
        for acc_pt, kind in ((eff, "doubling"), (G1.neg(eff), "infinity")):
            vmax = rng.randrange(22 * Q // 10, 23 * Q // 10)
            vmax = (vmax & ~(MASK29 << 29)) | (((1 << 29) - 2) << 29)
            reps = z_reps(vmax, 1)
            z = vmax % Q * RINV % Q
            assert one(acc_pt, z, 0, 0, reps[-4][1], p, neg) == kind and reps[-4][0] == vmax % Q < Q
            assert one(acc_pt, z, 6, 4, reps[2][1], p, neg) == kind
            assert one(acc_pt, z, 6, 0, reps[1][1], p, neg) == kind
        for xy in ((ONE, ONE), (7 * Q - 1, 5 * Q - 1)):
            qx, qy = p[0] * RR % Q, p[1] * RR % Q
            acc = [nform(xy[0]), nform(xy[1]), limbs(0)]
            fn, kind = lazy_judge(acc, qx, Q - qy if neg else qy, eff, stats)
            assert kind == "accumulator at infinity"
            C.add("jac_madd_lazy", acc + [limbs(qx), limbs(qy)], k=neg, fn=fn)
    # one chain: 300 additions of table points with signs into one accumulator, every intermediate judged
    acc_l, acc_pt, prev = [limbs(ONE), limbs(ONE), limbs(0)], None, None
    for step in range(300):
        i = rng.randrange(12)
        while i == prev:
            i = rng.randrange(12)
        prev, neg = i, rng.randrange(2)
        p = T[i]
        qx, qy = p[0] * RR % Q, p[1] * RR % Q
        acc_pt = B.add(acc_pt, G1.neg(p) if neg else p)
        fn, kind = lazy_judge(acc_l, qx, Q - qy if neg else qy, acc_pt, stats)
        assert kind == ("general" if step else "accumulator at infinity")
        C.add("jac_madd_lazy_chain", [limbs(0)] * 3 + [limbs(qx), limbs(qy)], k=neg, fn=fn)
        if step == 0:
            acc_l = [limbs(qx), nform(Q - qy if neg else qy), limbs(ONE)]
        else:
            m = madd_lazy_model(*(val(l) for l in acc_l), qx, Q - qy if neg else qy, LazyStats())
            acc_l = [nform(m[0]), nform(m[1]), [2 * x for x in nform(m[2] // 2)]]
    return npairs


_MADE = {}


def all_cases(host):
    """the case list (made once per kind), its counts and the statistics of the jac_madd_lazy model"""
    if host not in _MADE:
        C, stats = Cases(), LazyStats()
        field_cases(C, host)
        lazy_cases(C)
        curve_cases(C)
        npairs = madd_lazy_cases(C, stats)
        _MADE[host] = (C, stats, npairs)
    return _MADE[host]


def run_and_judge(exe, d, host, start=None):
    """write the cases, run the program, -> (complaints, stdout); the counts it prints must be the counts written, operation by operation"""
    C, stats, npairs = all_cases(host)
    cases, results = os.path.join(d, "fq_cases.bin"), os.path.join(d, "fq_results.bin")
    counts = C.write(cases)
    if os.path.exists(results):
        os.remove(results)
    out = start([exe, cases, results]) if start else subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert ("build host" if host else "build device") in out.stdout
    seen = {m[1]: int(m[2]) for m in re.finditer(r"^prim (\S+) cases (\d+)$", out.stdout, re.M)}
    assert sorted(seen) == sorted(OPS)
    for op in OPS:
        want = counts.get(op, 0)
        assert seen[op] == want, (op, seen[op], want)
        assert want > 0 or (not host and op in HOST_ONLY), "no case for " + op
    # conditions on the inputs: what the cases must have reached
    assert npairs >= 64 and counts["jac_madd_lazy_chain"] == 300
    assert all(n > 0 for n in stats.branch.values()), stats.branch
    assert all(n > 0 for n in stats.tight.values()), stats.tight
    return C.judge(results), out.stdout, counts, stats


def report(counts, stats):
    print("cases per operation:", ", ".join("%s %d" % (op, counts.get(op, 0)) for op in OPS))
    print("jac_madd_lazy branches:", stats.branch, " subtractions met within one q of zero:", stats.tight)
    print("largest seen, units of q (bound of the comment): " + ", ".join(
        "%s %.3f (%s)" % (k, stats.max[k] / Q, b) for k, b in (("X3", "5.86"), ("Y3", "4.52"), ("Z3", "2.22"), ("H", "8.02"), ("rr", "12.03"))))


def build_host(exe, extra=(), include_first=None):
    inc = (["-I", include_first] if include_first else []) + ["-I", CSRC]
    subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, *inc, "-x", "c++", os.path.join(NATIVE, "fq254_check.hip"), "-o", exe])


def build_device(exe, include_first=None):
    inc = (["-I", include_first] if include_first else []) + ["-I", CSRC]
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=" + ARCH, *inc, "-o", exe, os.path.join(NATIVE, "fq254_check.hip")])


@pytest.mark.parametrize("build", ["plain", "san"])
def test_fq254_host_at_its_bounds(tmp_path, build):
    exe = str(tmp_path / "fq254_check_host")
    build_host(exe, extra=SAN if build == "san" else ())
    bad, _, counts, stats = run_and_judge(exe, str(tmp_path), host=True)
    report(counts, stats)
    assert not bad, "%d complaints, the first: %s" % (len(bad), bad[:5])
    # the comment's bounds hold over everything the model saw
    assert stats.max["X3"] < 7 * Q and stats.max["Y3"] < 5 * Q and 10 * stats.max["Z3"] < 23 * Q


# one line of fq254.hpp each, judged against the contract its comments state
MUTANTS = {
    "H with one q less": ("const fq H = lz_sub<7>(U2, p.X);", "const fq H = lz_sub<6>(U2, p.X);"),
    "rr with one q less": ("const fq rr = lz_dbl(lz_sub<5>(S2, p.Y));", "const fq rr = lz_dbl(lz_sub<4>(S2, p.Y));"),
    "X3 with one q less": ("r.X = lz_sub2<4>(lz_mul(rr, rr), J, lz_dbl(V));", "r.X = lz_sub2<3>(lz_mul(rr, rr), J, lz_dbl(V));"),
    "fq_mul2 drops bit 29 of d": (
        "        for (int i = 0; i <= k; i++) {\n            acc += (u64)a.l[i] * b.l[k - i];\n            acc += (u64)c.l[i] * d.l[k - i];\n        }",
        "        for (int i = 0; i <= k; i++) {\n            acc += (u64)a.l[i] * b.l[k - i];\n            acc += (u64)c.l[i] * (d.l[k - i] & FQ_MASK);\n        }"),
}


def mutant_header(d, mutant):
    old, new = MUTANTS[mutant]
    with open(os.path.join(CSRC, "fq254.hpp")) as f:
        src = f.read()
    assert src.count(old) == 1, "the line this mutant changes is gone from fq254.hpp: " + old
    with open(os.path.join(d, "fq254.hpp"), "w") as f:
        f.write(src.replace(old, new))


def judge_mutant(bad, mutant):
    hit = sorted({op for op, _, _ in bad})
    assert hit, "no case notices: " + mutant
    if mutant.startswith("fq_mul2"):
        assert "fq_mul2" in hit, hit
    else:
        assert set(hit) <= {"jac_madd_lazy", "jac_madd_lazy_chain"} and "jac_madd_lazy" in hit, hit


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_fq254_bound_cases_catch_a_wrong_line_on_the_host(tmp_path, mutant):
    mutant_header(str(tmp_path), mutant)
    exe = str(tmp_path / "fq254_check_mutant")
    build_host(exe, include_first=str(tmp_path))          # "fq254.hpp" resolves to the copy
    bad, _, _, _ = run_and_judge(exe, str(tmp_path), host=True)
    judge_mutant(bad, mutant)


# ---------------------------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_fq254_device_at_its_bounds(tmp_path):
    exe = str(tmp_path / "fq254_check_device")
    build_device(exe)
    bad, _, counts, stats = run_and_judge(exe, str(tmp_path), host=False, start=lambda argv: run_latched("fq254_check", argv))
    report(counts, stats)
    assert not bad, "%d complaints, the first: %s" % (len(bad), bad[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_fq254_bound_cases_catch_a_wrong_line_on_the_device(tmp_path, mutant):
    mutant_header(str(tmp_path), mutant)
    exe = str(tmp_path / "fq254_check_mutant")
    build_device(exe, include_first=str(tmp_path))
    bad, _, _, _ = run_and_judge(exe, str(tmp_path), host=False, start=lambda argv: run_latched("fq254_check mutant", argv))
    judge_mutant(bad, mutant)
