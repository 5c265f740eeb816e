"""The verifier's Fiat-Shamir transcripts as device sponge chains ("verify_chain_dev"): the BN128-mode chain primitive on the device against its host
path word for word; whole BN128-mode and Goldilocks-mode texts, single and in batches, and one aggregated text, under knob 0 (host sponges) and knob 2
(one chain launch per call, long public-input vectors committed on the device): the same verdict, `where` and indices, the CPU checker's class, and
counters (zp_verify_counters) that say what ran where -- without them a silent fallback to the host would pass every comparison here."""
import contextlib
import copy
import json

import numpy as np
import pytest

import stark_verify_bn128_cases as BC
import stark_verify_cases as SC
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
from eigen_zeth_amd.stark import air as AIR, prover as PR, verifier_air as VA
from oracle import stark_verify as SV
from oracle.stark_cpu import CpuBackend

pytestmark = pytest.mark.gpu
R = SV.R_BN254
V = native


@pytest.fixture(scope="module")
def bn_tables():
    return bn254_poseidon_params(17)


@pytest.fixture(scope="module")
def p17(prover):
    prover.install_poseidon_bn254(17)
    return prover


@contextlib.contextmanager
def knob(prover, value):
    prover.set_tuning("verify_chain_dev", value)
    try:
        yield
    finally:
        prover.set_tuning("verify_chain_dev", 1)


def counted(prover, fn):
    """(what fn returns, how far each counter moved)"""
    before = native.verify_counters(prover)
    out = fn()
    after = native.verify_counters(prover)
    return out, {k: after[k] - before[k] for k in after}


NOTHING = {"launches": 0, "steps": 0, "digests": 0, "fallbacks": 0}


def test_the_knob_takes_0_1_2_only(prover):
    for bad in (-1, 3):
        with pytest.raises(native.ZpError):
            prover.set_tuning("verify_chain_dev", bad)
    prover.set_tuning("verify_chain_dev", 1)


# ---- the primitive: device words = host words
def random_chains(lengths, seed):
    """blocks, absorb, first of chains of these lengths: random elements below r, about a third of the steps bare, r - 1 and 0 among the elements"""
    rng = np.random.default_rng(seed)
    n = sum(lengths)
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(16 * n)]
    if n:
        vals[0], vals[-1] = R - 1, 0
    absorb = [int(rng.integers(0, 3) != 0) for _ in range(n)]
    first = [0]
    for l in lengths:
        first.append(first[-1] + l)
    return native.Prover._fr_words(vals).reshape(n, 16, 4), absorb, first


@pytest.mark.parametrize("lengths", [
    (2,), (3, 1), (2, 2, 3), (1, 2, 3, 2), (1, 2, 3, 1, 2, 3, 2),      # 1, 2, 3, 4, 7 chains: 3 -> 4 is the seam of three chains per workgroup
    (1, 9, 4),                                                          # one workgroup, three lengths: the predicated tail
    (3, 0, 2), (0, 0, 5, 0),                                            # chains of no steps between and around others
    (40,),
], ids=lambda l: "x".join(map(str, l)))
def test_primitive_on_the_device_gives_the_host_words(p17, bn_tables, lengths):
    blocks, absorb, first = random_chains(lengths, 1000 + sum(lengths) + len(lengths))
    host = native.poseidon_bn254_chains(blocks, absorb, first, bn_tables=bn_tables)
    got, moved = counted(p17, lambda: native.poseidon_bn254_chains(blocks, absorb, first, prover=p17))
    assert got.shape == host.shape == (sum(lengths), 16, 4)
    assert (got == host).all(), np.argwhere(got != host)[:4]
    assert moved == {"launches": 1, "steps": sum(lengths), "digests": 0, "fallbacks": 0}


def test_primitive_argument_errors_through_a_ctx(p17):
    blocks, absorb, first = random_chains((2,), 5)
    bad = blocks.copy()
    bad[1, 3] = native.Prover._fr_words([R])[0]
    for args in ((bad, absorb, first), (blocks, absorb, [1, 2]), (blocks, absorb, [0, 2, 1])):
        with pytest.raises(native.ZpError) as e:
            native.poseidon_bn254_chains(*args, prover=p17)
        assert e.value.code == -1
    got, moved = counted(p17, lambda: native.poseidon_bn254_chains(np.zeros((0, 16, 4), dtype=np.uint64), [], [0, 0, 0], prover=p17))
    assert got.shape == (0, 16, 4) and moved == NOTHING


# ---- BN128-hash mode
PICK = ("trace value", "fri0 value", "trace sibling word", "trace root", "trace root = r", "fri root", "evaluation at zeta", "evaluation at zeta w", "final-layer word",
        "final-layer word, header only", "public input", "params.logb", "hash relabelled gl", "index ^ 1", "publics shortened", "evaluations shortened",
        "fri roots shortened", "final layer shortened", "queries dropped", "queries dropped, header only", "stage2 root dropped",
        "last-layer FRI value, trusted openings", "trace value = p, trusted openings")
_bn = {}


def bn_case(prover, tables, bn_tables, name, seed=11):
    if name == "vair":
        return BC.make_vair_case(BC.cpu_backend(tables, bn_tables), tables)
    a = BC.SHAPES[name]
    air, tr, pub = SC.witness(name, a[0], seed)
    d = prover.upload(tr)
    text = prover.stark_prove_bn128(air.name, air.program(), d, [int(v) for v in pub], *a)
    d.free()
    return BC.Case(name, air.program(), PR.StarkParams(*a, hash="bn128"), text)


def bn_rows(prover, tables, bn_tables, name):
    """the case and (label, flags, text, the checker's class) of the honest text and of the picked mutations, a missing root among them: made once"""
    if name not in _bn:
        case = bn_case(prover, tables, bn_tables, name)
        muts = [("honest", 0, case.proof)] + [m for m in BC.single_field_mutations(case) if m[0] in PICK]
        muts.append(("trace root dropped", 0, BC.mutated(case.proof, ("roots", "trace"), None)))
        _bn[name] = (case, [(label, flags, PR.proof_to_json(m), BC.oracle_class(case, m, tables, bn_tables, flags)) for label, flags, m in muts])
    return _bn[name]


@pytest.mark.parametrize("name", BC.NAMES)
def test_bn128_texts_under_knob_0_and_2(p17, tables, bn_tables, name):
    case, rows = bn_rows(p17, tables, bn_tables, name)
    classes = set()
    for label, flags, text, want in rows:
        with knob(p17, 0):
            host, moved0 = counted(p17, lambda: native.stark_verify_bn128(case.program, text, case.params, flags, prover=p17))
        with knob(p17, 2):
            dev, moved2 = counted(p17, lambda: native.stark_verify_bn128(case.program, text, case.params, flags, prover=p17))
        assert dev == host, (name, label, dev, host)
        assert dev[0] == want, (name, label, dev, want)
        assert moved0 == NOTHING, (name, label, moved0)
        assert moved2["launches"] + moved2["fallbacks"] == 1, (name, label, moved2)      # a planned text is one launch, any other is counted
        classes.add(dev[0])
        if label == "honest":
            assert dev[0] == V.VERDICT_ACCEPT and dev[2] == BC.oracle_indices(case, tables, bn_tables)
            assert moved2["launches"] == 1 and moved2["steps"] > 0 and moved2["fallbacks"] == 0
            assert moved2["digests"] == (1 if name == "vair" else 0)
            assert name != "vair" or len(case.proof["publics"]) > 64
        if label in ("trace root dropped", "trace root = r", "stage2 root dropped"):
            assert dev[0] == V.VERDICT_MALFORMED and moved2 == {"launches": 0, "steps": 0, "digests": 0, "fallbacks": 1}, (name, label, moved2)
    assert {V.VERDICT_ACCEPT, V.VERDICT_OPENING, V.VERDICT_FRI, V.VERDICT_IDENTITY, V.VERDICT_INDICES, V.VERDICT_MALFORMED, V.VERDICT_PARAMS} <= classes
    # the default leaves BN128 mode on the host: the device lost to the parent library at 16 texts (profiles/verify_chains.json)
    _, moved = counted(p17, lambda: native.stark_verify_bn128(case.program, rows[0][2], case.params, prover=p17))
    assert moved == NOTHING


def test_bn128_batch_is_one_launch(p17, tables, bn_tables):
    cs = [bn_case(p17, tables, bn_tables, "chunk16", seed) for seed in (21, 22, 23, 24, 25)]
    texts = [c.text for c in cs]
    texts[1] = PR.proof_to_json(BC.mutated(cs[1].proof, ("queries", 3, "fri", 1, "values", 5), BC.bump))
    texts[3] = PR.proof_to_json(BC.mutated(cs[3].proof, ("evals", "zw", 2, 0), BC.bump))
    texts[4] = PR.proof_to_json(BC.mutated(cs[4].proof, ("roots", "quotient"), None))
    case = cs[0]
    with knob(p17, 0):
        single = [native.stark_verify_bn128(case.program, t, case.params, prover=p17)[0] for t in texts]
        host, moved0 = counted(p17, lambda: native.stark_verify_batch_bn128(case.program, texts, case.params, prover=p17))
    assert single == [0, V.VERDICT_OPENING, 0, V.VERDICT_IDENTITY, V.VERDICT_MALFORMED] and host == single and moved0 == NOTHING
    with knob(p17, 2):
        for threads in (0, 3):
            dev, moved = counted(p17, lambda: native.stark_verify_batch_bn128(case.program, texts, case.params, prover=p17, threads=threads))
            assert dev == single
            assert moved["launches"] == 1 and moved["fallbacks"] == 1 and moved["digests"] == 0 and moved["steps"] > 0
        assert [native.stark_verify_bn128(case.program, t, case.params, prover=p17)[0] for t in texts] == single


# ---- Goldilocks mode under knob 2
GL_PICK = ("trace value", "index ^ 1", "pow_nonce + 1", "pow_nonce dropped", "final-layer word", "final-layer word, header only", "evaluation at zeta",
           "quotient evaluation", "trace-root word", "fri-root word", "public input", "params.logb", "publics shortened", "final layer shortened",
           "queries dropped, header only", "stage2 root dropped", "last-layer FRI value, trusted openings")
_gl = {}


def gl_case(prover, tables, name, seed=11):
    if name == "vair":      # more than 64 public inputs: the binary tree over rows of 8, on the device
        return SC.make_vair_case(CpuBackend(*tables), *tables)
    a = SC.SHAPES[name]
    air, tr, pub = SC.witness(name, a[0], seed)
    d = prover.upload(tr)
    text = prover.stark_prove(air.name, air.program(), d, [int(v) for v in pub], *a)
    d.free()
    return SC.Case(name, air.program(), PR.StarkParams(*a[:5], pow_bits=a[5]), text)


@pytest.mark.parametrize("name", list(SC.SHAPES) + ["vair"])
def test_goldilocks_texts_under_knob_0_and_2(prover, tables, name):
    if name not in _gl:
        _gl[name] = gl_case(prover, tables, name)
    case = _gl[name]
    rows = [("honest", 0, case.proof)] + [m for m in SC.single_field_mutations(case) if m[0] in GL_PICK]
    for label, flags, m in rows:
        text = PR.proof_to_json(m)
        with knob(prover, 0):
            host, moved0 = counted(prover, lambda: native.stark_verify(case.program, text, case.params, flags, prover=prover))
        with knob(prover, 2):
            dev, moved2 = counted(prover, lambda: native.stark_verify(case.program, text, case.params, flags, prover=prover))
        assert dev == host, (name, label, dev, host)
        assert dev[0] == SC.oracle_class(case, m, *tables, flags), (name, label, dev)
        assert moved0 == NOTHING and moved2["launches"] + moved2["fallbacks"] == 1, (name, label, moved0, moved2)
        if label == "honest":
            assert dev[0] == V.VERDICT_ACCEPT and dev[2] == SC.oracle_indices(case, *tables)
            assert moved2["launches"] == 1 and moved2["steps"] > 0 and moved2["digests"] == (1 if name == "vair" else 0)
        if label == "pow_nonce + 1":          # the grinding permutation stays on the host: the chain ran, the verdict is the nonce's
            assert dev[0] == V.VERDICT_POW and moved2["launches"] == 1
        if label == "pow_nonce dropped":
            assert dev[0] == V.VERDICT_POW and moved2["fallbacks"] == 1
        if label == "final-layer word, header only":
            assert flags == V.VERIFY_HEADER_ONLY and moved2["launches"] == 1
    # the default leaves Goldilocks mode on the host
    _, moved = counted(prover, lambda: native.stark_verify(case.program, case.text, case.params, prover=prover))
    assert moved == NOTHING


def test_goldilocks_batch_is_one_launch(prover, tables):
    cs = [gl_case(prover, tables, "chunk16", seed) for seed in (21, 22, 23)]
    texts = [c.text for c in cs]
    texts[1] = PR.proof_to_json(SC.mutated(cs[1].proof, ("evals", "zw", 2, 0), SC.bump))
    case = cs[0]
    with knob(prover, 0):
        host = native.stark_verify_batch(case.program, texts, case.params, prover=prover)
    assert host == [0, V.VERDICT_IDENTITY, 0]
    with knob(prover, 2):
        dev, moved = counted(prover, lambda: native.stark_verify_batch(case.program, texts, case.params, prover=prover))
    assert dev == host and moved["launches"] == 1 and moved["fallbacks"] == 0


def test_aggregated_text_outer_stark_on_the_chain_inner_headers_read(prover, tables):
    """one aggregation over two chunk16 proofs of 2^6 rows: the outer STARK's transcript is a chain, the inner headers' transcripts are still READ"""
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    hip = HipBackend(prover=prover)
    air = AIR.get_air("chunk16")
    params = PR.StarkParams(6, 1, 2, 3, 4, pow_bits=4)
    proofs = []
    for seed in (3, 4):
        tr, pub = native.synth_trace(air.trace_kind, 6, air.width, seed)
        proofs.append(json.loads(PR.proof_to_json(PR.prove(air, tr, pub, params, hip))))
    shape = VA.Shape.of_proof(proofs[0], 2)
    vair = VA.verifier_air(shape, *tables)
    d_trace, pubs = VA.build_witness(shape, proofs, hip, air.digest_words())
    ap = VA.aggregation_params(shape, n_queries=5, fri_final_log=3)
    agg = {"shape": shape.to_dict(), "inner": [{k: copy.deepcopy(v) for k, v in p.items() if k != "queries"} for p in proofs],
           "stark": json.loads(hip.prove_native(vair, d_trace, pubs, ap))}
    statements = [(None, air.program(), params, 0), (shape.to_dict(), vair.program(), ap, shape.n_slots())]
    outer_bad, inner_bad = copy.deepcopy(agg), copy.deepcopy(agg)
    outer_bad["stark"]["evals"]["z"][0][1] ^= 1
    inner_bad["inner"][1]["evals"]["z"][2][1] ^= 1
    want = [(V.VERDICT_ACCEPT, -1), (V.VERDICT_IDENTITY, -1), (V.VERDICT_TRANSCRIPT, 0)]
    texts = [json.dumps(o) for o in (agg, outer_bad, inner_bad)]
    with knob(prover, 0):
        host, moved0 = counted(prover, lambda: [native.aggregate_verify(statements, t, prover=prover) for t in texts])
    assert host == want and moved0 == NOTHING
    with knob(prover, 2):
        for t, w in zip(texts, want):
            dev, moved = counted(prover, lambda: native.aggregate_verify(statements, t, prover=prover))
            assert dev == w and moved["launches"] == 1 and moved["fallbacks"] == 0 and moved["digests"] == 1      # (the verifier AIR has > 64 public inputs)
        dev, moved = counted(prover, lambda: native.aggregate_verify_batch(statements, texts, prover=prover))
        assert dev == [w[0] for w in want] and moved["launches"] == 1 and moved["digests"] == 3
