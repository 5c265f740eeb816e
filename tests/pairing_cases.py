"""Inputs shared by tests/test_pairing_host.py and tests/test_gpu_pairing.py: synthetic Groth16 instances without a circuit, word packing, the
expected GT value of e(aG1, bG2) without a pairing per case, and the classes of spoiled proofs.  Expectations come from the checker
(oracle/bn254_pairing.py, oracle/naive_bn254.py, oracle/groth16_verify.py) and identities over it, never from the library."""
import random

import numpy as np

from oracle import bn254_pairing as BP
from oracle import naive_bn254 as B
from test_pairing254 import e1, g1_words, g2_words, off_subgroup_point, unwords, words

Q, R = B.Q, B.R
ACCEPT, PUBLICS, POINT, PAIRING = 0, 10, 12, 13


def gt_of(a, b):
    """e(aG1, bG2) = e(G1, G2)^(ab)"""
    return BP.f_pow(e1(), a * b % R)


def gt_ints(gt_row):
    return [unwords(gt_row[k]) for k in range(12)]


class Key:
    """key = (alpha G1, beta G2, gamma G2, delta G2, [s_j G1]) from seeded scalars"""

    def __init__(self, rng, n_ic, small=False):
        draw = (lambda: rng.randrange(2, 1 << 24)) if small else (lambda: rng.randrange(1, R))
        self.alpha, self.beta, self.gamma, self.delta = draw(), draw(), draw(), draw()
        self.s = [draw() for _ in range(n_ic)]
        self.vk = {"alpha1": B.mul(B.G, self.alpha), "beta2": B.mul_g2(B.G2, self.beta), "gamma2": B.mul_g2(B.G2, self.gamma),
                   "delta2": B.mul_g2(B.G2, self.delta), "ic": [B.mul(B.G, s) for s in self.s]}
        self.n_ic = n_ic

    def words(self):
        return np.array(g1_words(self.vk["alpha1"]) + g2_words(self.vk["beta2"]) + g2_words(self.vk["gamma2"]) + g2_words(self.vk["delta2"]) +
                        [w for p in self.vk["ic"] for w in g1_words(p)], dtype=np.uint32)

    def instance(self, rng, small=True):
        """(proof dict, publics): a, b and the publics drawn, c = (ab - alpha beta - x gamma)/delta mod r with x = s_0 + sum pub_j s_j"""
        draw = (lambda: rng.randrange(2, 1 << 20)) if small else (lambda: rng.randrange(1, R))
        a, b = draw(), draw()
        pubs = [rng.randrange(R) if not small else rng.randrange(1 << 32) for _ in range(self.n_ic - 1)]
        x = (self.s[0] + sum(p * s for p, s in zip(pubs, self.s[1:]))) % R
        c = (a * b - self.alpha * self.beta - x * self.gamma) * pow(self.delta, -1, R) % R
        return {"pi_a": B.mul(B.G, a), "pi_b": B.mul_g2(B.G2, b), "pi_c": B.mul(B.G, c)}, pubs


def proof_words(proof):
    return g1_words(proof["pi_a"]) + g2_words(proof["pi_b"]) + g1_words(proof["pi_c"])


# every class of spoiled proof: name -> (function of (proof words list, publics list, rng) -> (words, publics), expected verdict)
def _set(w, at, vals):
    w = list(w)
    w[at:at + len(vals)] = vals
    return w


SPOILS = {
    "public+1": (lambda w, p, rng: (w, [(p[0] + 1) % R] + p[1:]), PAIRING),
    "pi_a other": (lambda w, p, rng: (_set(w, 0, g1_words(B.mul(B.G, rng.randrange(2, 1 << 20)))), p), PAIRING),
    "pi_b other": (lambda w, p, rng: (_set(w, 16, g2_words(B.mul_g2(B.G2, rng.randrange(2, 1 << 20)))), p), PAIRING),
    "pi_c other": (lambda w, p, rng: (_set(w, 48, g1_words(B.mul(B.G, rng.randrange(2, 1 << 20)))), p), PAIRING),
    "public=r": (lambda w, p, rng: (w, [R] + p[1:]), PUBLICS),
    "coordinate=q": (lambda w, p, rng: (_set(w, 48, words(Q)), p), POINT),
    "pi_a off curve": (lambda w, p, rng: (_set(w, 0, g1_words((1, 3))), p), POINT),
    "pi_b off subgroup": (lambda w, p, rng: (_set(w, 16, g2_words(off_subgroup_point())), p), POINT),
}


def pub_words(pubs_list, n_pub):
    flat = [v for row in pubs_list for v in row]
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in flat] or [[0] * 4], dtype=np.uint64)


def proof_from_words(w):
    g1 = lambda o: None if not any(w[o:o + 16]) else (unwords(w[o:o + 8]), unwords(w[o + 8:o + 16]))
    b = [unwords(w[16 + 8 * k:24 + 8 * k]) for k in range(4)]
    return {"pi_a": g1(0), "pi_b": None if not any(b) else ((b[0], b[1]), (b[2], b[3])), "pi_c": g1(48)}


def batch_with_spoils(seed, n, n_ic=2, positions=None):
    """a key and n valid small-scalar instances, spoiled at `positions` ({index: spoil name}): (Key, u32[n][64], publics lists, expected verdicts)"""
    rng = random.Random(seed)
    key = Key(rng, n_ic, small=True)
    rows, pubs, want = [], [], []
    for i in range(n):
        proof, p = key.instance(rng)
        w = proof_words(proof)
        name = (positions or {}).get(i)
        if name:
            w, p = SPOILS[name][0](w, p, rng)
        rows.append(w)
        pubs.append(p)
        want.append(SPOILS[name][1] if name else ACCEPT)
    return key, np.array(rows, dtype=np.uint32), pubs, want
