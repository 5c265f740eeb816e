"""zp_aggregate_verify / zp_aggregate_verify_batch on the MI355X: proofs made on the HIP backend as tests/test_gpu_verifier_air.py makes them (two
chunk16 proofs at 2^6 rows, their aggregation, the level-2 tree over two such aggregations, and one level-1 over two chunk64 proofs at 2^10 rows), judged
through a ctx -- the openings of the outer STARK in the one launch of the query phase, the fixed columns of every header from
zp_program_fixed_eval_ext_batch -- and with ctx = NULL: the same verdicts, and the checker's (oracle/aggregate_verify.py)."""
import copy
import json

import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR
from eigen_zeth_amd.stark import verifier_air as VA
from eigen_zeth_amd.stark.backend_hip import HipBackend
from oracle import aggregate_verify as AV
from oracle import stark_verify as V

pytestmark = pytest.mark.gpu
ACCEPT, OPENING, TRANSCRIPT = native.VERDICT_ACCEPT, native.VERDICT_OPENING, native.VERDICT_TRANSCRIPT


def strip_paths(proof):
    return {k: copy.deepcopy(v) for k, v in proof.items() if k != "queries"}


def level_one(hip, tables, airname, logn, seeds, nq_inner=4):
    """(air, params, shape, vair, ap, text object) of one aggregation over two proofs made on the device"""
    air = AIR.get_air(airname)
    params = PR.StarkParams(logn, 1, 2, 3, nq_inner, pow_bits=4)
    proofs = []
    for seed in seeds:
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, seed)
        proofs.append(json.loads(PR.proof_to_json(PR.prove(air, tr, pub, params, hip))))
    shape = VA.Shape.of_proof(proofs[0], 2)
    vair = VA.verifier_air(shape, *tables)
    d_trace, pubs = VA.build_witness(shape, proofs, hip, air.digest_words())
    ap = VA.aggregation_params(shape, n_queries=5, fri_final_log=3)
    stark = json.loads(hip.prove_native(vair, d_trace, pubs, ap))
    return air, params, shape, vair, ap, {"shape": shape.to_dict(), "inner": [strip_paths(p) for p in proofs], "stark": stark}


@pytest.fixture(scope="module")
def tree(prover, tables):
    hip = HipBackend(prover=prover)
    air, params, shape1, vair1, ap1, A = level_one(hip, tables, "chunk16", 6, (3, 4))
    B = level_one(hip, tables, "chunk16", 6, (5, 6))[5]
    shape2 = VA.Shape.of_proof(A["stark"], 2)
    vair2 = VA.verifier_air(shape2, *tables)
    d2, pubs2 = VA.build_witness(shape2, [A["stark"], B["stark"]], hip, vair1.digest_words())
    ap2 = VA.aggregation_params(shape2, n_queries=4, fri_final_log=3)
    top = {"shape": shape2.to_dict(), "level": 2, "inner": [strip_paths(A["stark"]), strip_paths(B["stark"])],
           "children": [{"shape": A["shape"], "inner": A["inner"]}, {"shape": B["shape"], "inner": B["inner"]}],
           "stark": json.loads(hip.prove_native(vair2, d2, pubs2, ap2))}
    statements = [(None, air.program(), params, 0), (shape1.to_dict(), vair1.program(), ap1, shape1.n_slots()), (shape2.to_dict(), vair2.program(), ap2, shape2.n_slots())]
    programs = {shape1.key(): (vair1.program(), ap1), shape2.key(): (vair2.program(), ap2)}

    def checker(agg):
        try:
            return bool(AV.verify_tree(agg, air.program(), V.expectation(params.to_dict()), tables[0], tables[1],
                                       lambda d: (programs[VA.Shape.from_dict(d).key()][0], VA.Shape.from_dict(d).n_slots()),
                                       lambda d: V.expectation(programs[VA.Shape.from_dict(d).key()][1].to_dict())))
        except (V.Reject, KeyError, ValueError, IndexError, TypeError):
            return False
    return statements, A, top, checker


def both(statements, obj, prover, flags=0):
    """the verdict through the ctx, which must be the host's"""
    text = json.dumps(obj)
    got = native.aggregate_verify(statements, text, flags, prover=prover)
    assert got == native.aggregate_verify(statements, text, flags)
    return got


def test_level_one_and_level_two_verdicts_with_and_without_a_ctx(prover, tree):
    statements, A, top, checker = tree
    for obj in (A, top):
        assert both(statements, obj, prover) == (ACCEPT, -1) and checker(obj)
    bad = copy.deepcopy(top)
    bad["children"][1]["inner"][0]["evals"]["z"][2][1] ^= 1
    assert both(statements, bad, prover) == (TRANSCRIPT, 2) and not checker(bad)
    bad = copy.deepcopy(top)
    bad["stark"]["queries"][3]["fri"][0]["values"][1] ^= 1
    assert both(statements, bad, prover) == (OPENING, -1) and not checker(bad)
    assert both(statements, bad, prover, native.VERIFY_HEADER_ONLY) == (ACCEPT, -1)
    bad = copy.deepcopy(A)
    bad["stark"]["queries"][0]["trace"]["path"][2][3] ^= 1
    assert both(statements, bad, prover) == (OPENING, -1) and not checker(bad)


def test_batch_gives_mixed_verdicts(prover, tree):
    statements, A, top, _ = tree
    bad = copy.deepcopy(top)
    bad["inner"][1]["fri"]["final"][2][5] ^= 1
    worse = copy.deepcopy(A)
    worse["stark"]["queries"][1]["quotient"]["values"][0] ^= 1
    texts = [json.dumps(o) for o in (top, bad, A, worse, top)]
    want = [ACCEPT, TRANSCRIPT, ACCEPT, OPENING, ACCEPT]
    assert native.aggregate_verify_batch(statements, texts, prover=prover) == want
    assert native.aggregate_verify_batch(statements, texts) == want


def test_the_kernel_carries_every_header_of_the_tree(prover, tree):
    """fixed_eval_dev_min = 0: the fixed columns of the outer STARK and of all six headers of the level-2 tree come from the device kernels"""
    statements, _, top, _ = tree
    prover.set_tuning("fixed_eval_dev_min", 0)
    try:
        assert native.aggregate_verify(statements, json.dumps(top), prover=prover) == (ACCEPT, -1)
        bad = copy.deepcopy(top)
        bad["stark"]["evals"]["z"][0][1] ^= 1
        assert native.aggregate_verify(statements, json.dumps(bad), prover=prover) == (native.VERDICT_IDENTITY, -1)
    finally:
        prover.set_tuning("fixed_eval_dev_min", -1)
    prover.set_tuning("fixed_eval_dev_min", 2**31 - 1)
    try:
        assert native.aggregate_verify(statements, json.dumps(top), prover=prover) == (ACCEPT, -1)
    finally:
        prover.set_tuning("fixed_eval_dev_min", -1)


def test_level_one_over_two_chunk64_proofs_of_1024_rows(prover, tables):
    hip = HipBackend(prover=prover)
    air, params, shape, vair, ap, agg = level_one(hip, tables, "chunk64", 10, (11, 12))
    statements = [(None, air.program(), params, 0), (shape.to_dict(), vair.program(), ap, shape.n_slots())]
    plain = {"kind": "aggregated", "inner": agg["inner"], "stark": agg["stark"]}
    for knob in (0, -1):
        prover.set_tuning("fixed_eval_dev_min", knob)
        try:
            assert both(statements, agg, prover) == (ACCEPT, -1)
            assert both(statements, plain, prover) == (ACCEPT, -1)
        finally:
            prover.set_tuning("fixed_eval_dev_min", -1)
    args = (air.program(), vair.program(), tables[0], tables[1], V.expectation(params.to_dict()), V.expectation(ap.to_dict()), shape.n_slots())
    assert AV.verify(plain, *args)
    bad = copy.deepcopy(plain)
    bad["inner"][0]["pow_nonce"] ^= 1
    assert both(statements, bad, prover) == (TRANSCRIPT, 0)
    with pytest.raises(V.Reject):
        AV.verify(bad, *args)
