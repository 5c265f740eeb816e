"""zp_pairing_bn254, zp_pairing_check_bn254, zp_groth16_verify and zp_groth16_verify_batch with ctx = NULL: the host path of csrc/pairing.hip, which
runs the functions the kernels run.  Expected values come from the checker (oracle/bn254_pairing.py, oracle/groth16_verify.py) and from identities
over it (e(aG1, bG2) = e(G1, G2)^(ab)); inputs are synthetic Groth16 instances without a circuit (tests/pairing_cases.py), the points of the
reference's key (tests/golden/ref_vk.json) and the reference's own proof fixture."""
import itertools
import json
import os
import random

import numpy as np
import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.service import groth16 as G16
from oracle import bn254_pairing as BP
from oracle import groth16_verify as GV
from oracle import naive_bn254 as B
from pairing_cases import ACCEPT, PAIRING, POINT, PUBLICS, SPOILS, Key, batch_with_spoils, gt_ints, gt_of, proof_from_words, proof_words
from test_field_corners import ROOT
from test_pairing254 import g1_words, g2_words, off_subgroup_point, ref_vk_points, words

Q, R = B.Q, B.R


def test_verdict_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "zeth_prover.h")).read()
    assert "ZP_VERDICT_POINT = 12" in hdr and "ZP_VERDICT_PAIRING = 13" in hdr and "ZP_VERDICT_PUBLICS = 10" in hdr
    assert (native.VERDICT_PUBLICS, native.VERDICT_POINT, native.VERDICT_PAIRING) == (PUBLICS, POINT, PAIRING) and native.VERDICT_ACCEPT == ACCEPT


def test_pairing_equals_the_checker_word_for_word():
    rng = random.Random(0xE1)
    ab = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(8)]
    pts = [(B.mul(B.G, a), B.mul_g2(B.G2, b)) for a, b in ab]
    gt, st = native.pairing_bn254([g1_words(p) for p, _ in pts], [g2_words(q) for _, q in pts])
    assert st.tolist() == [0] * 8
    for j, (p, q) in enumerate(pts):
        assert gt_ints(gt[j]) == BP.pairing(q, p), j


@pytest.mark.parametrize("threads", [1, 3])
def test_64_pairs_equal_powers_of_e1(threads):
    rng = random.Random(0xE2)
    ab = [(rng.randrange(1, 1 << 16), rng.randrange(1, 1 << 16)) for _ in range(60)] + [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(4)]
    gt, st = native.pairing_bn254([g1_words(B.mul(B.G, a)) for a, _ in ab], [g2_words(B.mul_g2(B.G2, b)) for _, b in ab], threads=threads)
    assert not st.any()
    for j, (a, b) in enumerate(ab):
        assert gt_ints(gt[j]) == gt_of(a, b), j


def test_bilinear_and_non_degenerate_on_the_reference_key():
    g1s, g2s = ref_vk_points()
    P, Q2 = g1s[0], g2s[0]
    gt, st = native.pairing_bn254([g1_words(P), g1_words(B.mul(P, 2)), g1_words(P), g1_words(g1s[1])],
                                  [g2_words(Q2), g2_words(Q2), g2_words(B.mul_g2(Q2, 2)), g2_words(g2s[2])])
    assert not st.any()
    e = gt_ints(gt[0])
    assert e != BP.ONE and e == BP.pairing(Q2, P)
    assert gt_ints(gt[1]) == BP.f_mul(e, e) == gt_ints(gt[2])
    assert gt_ints(gt[3]) not in (BP.ONE, e)


def test_every_status_code():
    off = off_subgroup_point()
    g1 = [g1_words(None), g1_words(B.G), words(Q) + words(2), g1_words(B.G), g1_words((1, 3)), g1_words(B.G), g1_words(B.G), g1_words(B.mul(B.G, 3))]
    g2 = [g2_words(B.G2), g2_words(None), g2_words(B.G2), words(0) + words(Q) + words(1) + words(1), g2_words(B.G2), g2_words(((1, 2), (3, 4))), g2_words(off),
          g2_words(B.mul_g2(B.G2, 5))]
    gt, st = native.pairing_bn254(g1, g2)
    assert st.tolist() == [0, 0, 1, 1, 2, 2, 3, 0]
    assert gt_ints(gt[0]) == BP.ONE == gt_ints(gt[1])                  # infinity on either side: 1
    for j in range(2, 7):
        assert not gt[j].any()                                          # refused: all-zero
    assert gt_ints(gt[7]) == gt_of(3, 5)                                # the neighbour of refused pairs is right


def test_pairing_check():
    rng = random.Random(0xE3)
    a = rng.randrange(1, R)
    P, Q2 = B.G, B.mul_g2(B.G2, 7)
    neg = lambda p: (p[0], (-p[1]) % Q)
    good = ([g1_words(B.mul(P, a)), g1_words(neg(P))], [g2_words(Q2), g2_words(B.mul_g2(Q2, a))])
    assert native.pairing_check_bn254(*good) is True
    assert native.pairing_check_bn254([g1_words(B.mul(P, (a + 1) % R)), g1_words(neg(P))], good[1]) is False
    assert native.pairing_check_bn254(np.zeros((0, 16), dtype=np.uint32), np.zeros((0, 32), dtype=np.uint32)) is True
    assert native.pairing_check_bn254(good[0] + [g1_words((1, 3))], good[1] + [g2_words(None)]) is False          # one invalid point
    assert native.pairing_check_bn254(good[0] + [g1_words(None)], good[1] + [g2_words(B.G2)]) is True             # a pair with infinity changes nothing
    # more pairs than threads: 40 pairs (a_j P, Q) and one (-(sum a_j) P, Q)
    aj = [rng.randrange(1, 1 << 20) for _ in range(40)]
    g1 = [g1_words(B.mul(P, x)) for x in aj] + [g1_words(neg(B.mul(P, sum(aj))))]
    for threads in (1, 3, 16):
        assert native.pairing_check_bn254(g1, [g2_words(Q2)] * 41, threads=threads) is True
    assert native.pairing_check_bn254(g1[:-1] + [g1_words(neg(B.mul(P, sum(aj) + 1)))], [g2_words(Q2)] * 41, threads=3) is False


@pytest.mark.parametrize("n_ic", [1, 2, 5])
def test_groth16_accepts_synthetic_instances_and_classes_every_mutation(n_ic):
    rng = random.Random(0x6160 + n_ic)
    key = Key(rng, n_ic)
    proof, pubs = key.instance(rng, small=False)
    assert GV.verify(key.vk, proof, pubs)                               # the checker accepts the construction
    vk, w = key.words(), proof_words(proof)
    assert native.groth16_verify(vk, w, pubs) == ACCEPT
    for name, (spoil, want) in SPOILS.items():
        if name.startswith("public") and n_ic == 1:
            continue
        w2, p2 = spoil(w, pubs, rng)
        assert native.groth16_verify(vk, w2, p2) == want, name
    if n_ic > 1:
        assert not GV.verify(key.vk, proof, [(pubs[0] + 1) % R] + pubs[1:])
        # PUBLICS comes before POINT
        assert native.groth16_verify(vk, SPOILS["pi_a off curve"][0](w, pubs, rng)[0], [R] + pubs[1:]) == PUBLICS
    # pi_a at infinity: whatever the product of Miller loops says
    neg = lambda p: (p[0], (-p[1]) % Q)
    vkx = key.vk["ic"][0]
    for p, ic in zip(pubs, key.vk["ic"][1:]):
        vkx = B.add(vkx, B.mul(ic, p))
    f = BP.f_mul(BP.f_mul(BP.miller(proof["pi_b"], None), BP.miller(key.vk["beta2"], neg(key.vk["alpha1"]))),
                 BP.f_mul(BP.miller(key.vk["gamma2"], neg(vkx)), BP.miller(key.vk["delta2"], neg(proof["pi_c"]))))
    want = ACCEPT if BP.final_exp(f) == BP.ONE else PAIRING
    assert native.groth16_verify(vk, [0] * 16 + w[16:], pubs) == want == PAIRING


def test_200_random_single_word_mutations_agree_with_the_checker():
    """a random word of the proof replaced by a random word: accept / reject as oracle/groth16_verify.verify has it.  The checker's Miller values of the
    parts a mutation leaves alone are computed once (its verdict is a product of Miller values: BP.miller and BP.final_exp are the checker)"""
    rng = random.Random(0x200)
    key = Key(rng, 2)
    proof, pubs = key.instance(rng, small=False)
    vk, w = key.words(), proof_words(proof)
    neg = lambda p: (p[0], (-p[1]) % Q)
    vkx = B.add(key.vk["ic"][0], B.mul(key.vk["ic"][1], pubs[0]))
    fixed = BP.f_mul(BP.miller(key.vk["beta2"], neg(key.vk["alpha1"])), BP.miller(key.vk["gamma2"], neg(vkx)))
    m_c = BP.miller(key.vk["delta2"], neg(proof["pi_c"]))
    assert BP.final_exp(BP.f_mul(BP.f_mul(fixed, m_c), BP.miller(proof["pi_b"], proof["pi_a"]))) == BP.ONE

    def checker(p):          # oracle/groth16_verify.verify with the untouched factors reused
        if not (B.on_curve(p["pi_a"]) and B.on_curve(p["pi_c"])):
            return False
        mc = m_c if p["pi_c"] == proof["pi_c"] else BP.miller(key.vk["delta2"], neg(p["pi_c"]))
        return BP.final_exp(BP.f_mul(BP.f_mul(fixed, mc), BP.miller(p["pi_b"], p["pi_a"]))) == BP.ONE

    mutants, left_out = [], 0
    while len(mutants) < 200:
        at, val = rng.randrange(64), rng.getrandbits(32)
        if val == w[at]:
            continue
        mutants.append(w[:at] + [val] + w[at + 1:])
    verdicts = native.groth16_verify_batch(vk, np.array(mutants, dtype=np.uint32), [pubs] * 200, threads=0)
    assert GV.verify(key.vk, proof_from_words(mutants[0]), pubs) == checker(proof_from_words(mutants[0]))          # the shortcut is the checker
    for m, v in zip(mutants, verdicts):
        p = proof_from_words(m)
        b = p["pi_b"]
        if b is not None and all(c < Q for c in b[0] + b[1]) and B.on_curve_g2(b) and B.mul_g2(b, R) is not None:
            left_out += 1          # on the twist, outside the subgroup: the checker does not test that
            continue
        assert (v == ACCEPT) == checker(p), (m, v)
    assert left_out <= 2           # at most 1 % of the mutants


def test_bad_key_and_bad_arguments_are_errors():
    rng = random.Random(0xBAD)
    key = Key(rng, 2, small=True)
    proof, pubs = key.instance(rng)
    vk, w = key.words(), proof_words(proof)
    assert native.groth16_verify(vk, w, pubs) == ACCEPT
    for at, vals in ((0, g1_words((1, 3))), (0, [0] * 16), (16, g2_words(off_subgroup_point())), (48, [0] * 32), (80, g2_words(((1, 2), (3, 4)))),
                     (112 + 16, words(Q) + words(1))):
        bad = vk.copy()
        bad[at:at + len(vals)] = vals
        with pytest.raises(native.ZpError) as e:
            native.groth16_verify(bad, w, pubs)
        assert e.value.code == -1
    lib = native.load_library()
    verdict = np.zeros(1, dtype=np.int32)
    p = np.array(w, dtype=np.uint32)
    assert lib.zp_groth16_verify(None, vk.ctypes.data, 0, p.ctypes.data, None, verdict.ctypes.data_as(native.C.POINTER(native.C.c_int32))) == -1
    assert lib.zp_groth16_verify(None, None, 2, p.ctypes.data, None, verdict.ctypes.data_as(native.C.POINTER(native.C.c_int32))) == -1


def test_reference_fixture_is_pairing_under_all_36_role_assignments():
    g1, g2 = ref_vk_points()
    pr = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_proof.json")))
    pub = int(json.load(open(os.path.join(ROOT, "tests", "golden", "ref_public_input.json")))[0])
    proof = {"pi_a": (int(pr["pi_a"]["x"]), int(pr["pi_a"]["y"])),
             "pi_b": ((int(pr["pi_b"]["x"][0]), int(pr["pi_b"]["x"][1])), (int(pr["pi_b"]["y"][0]), int(pr["pi_b"]["y"][1]))),
             "pi_c": (int(pr["pi_c"]["x"]), int(pr["pi_c"]["y"]))}
    seen = 0
    for (ia, i0, i1) in itertools.permutations(range(3), 3):
        for (jb, jg, jd) in itertools.permutations(range(3), 3):
            vk = {"alpha1": g1[ia], "beta2": g2[jb], "gamma2": g2[jg], "delta2": g2[jd], "ic": [g1[i0], g1[i1]]}
            assert G16.verify(vk, proof, [pub]) == PAIRING, (ia, i0, i1, jb, jg, jd)
            seen += 1
    assert seen == 36


@pytest.mark.parametrize("threads", [1, 3])
def test_batch_returns_the_single_call_verdicts(threads):
    key, rows, pubs, want = batch_with_spoils(0xBA7, 7, positions={2: "pi_c other", 5: "pi_b off subgroup"})
    vk = key.words()
    assert native.groth16_verify_batch(vk, rows, pubs, threads=threads) == want == [native.groth16_verify(vk, r, p) for r, p in zip(rows, pubs)]
    assert want.count(ACCEPT) == 5


def test_dict_forms():
    rng = random.Random(0xD1C7)
    key = Key(rng, 3, small=True)
    proof, pubs = key.instance(rng)
    assert (G16.vk_words(key.vk) == key.words()).all() and G16.proof_words(proof).tolist() == proof_words(proof)
    assert G16.verify(key.vk, proof, pubs) == ACCEPT
    other, _ = key.instance(rng)
    assert G16.verify_batch(key.vk, [proof, other, proof], [pubs, pubs, [pubs[0], R]]) == [ACCEPT, PAIRING, PUBLICS]
    assert G16.verify_batch(key.vk, [], []) == []
