"""The Groth16 verifier at the end of the product's own chain, on the machine that makes the proofs: a proof zp_groth16_prove made on the GPU is
judged by zp_groth16_verify through the same ctx, and the engine's final proof passes EngineConfig(verify_final=True).  The verifier itself is host
code (csrc/pairing.hip); what runs on the GPU here is the prover whose output it judges."""
import pytest

import r1cs_cases as RC
from eigen_zeth_amd import native
from eigen_zeth_amd.service import groth16 as G16
from oracle import groth16_verify as GV
from oracle import naive_bn254 as B
from pairing_cases import ACCEPT, PAIRING, POINT, PUBLICS

pytestmark = pytest.mark.gpu
R = G16.R


def test_the_product_s_own_proof_is_accepted(prover):
    """zp_groth16_prove on the small circuit S1 under a seeded key: ACCEPT with its public inputs, PAIRING with one bumped, PUBLICS with one = r,
    POINT with pi_c moved off the curve; the checker agrees on accept / reject"""
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    prover.install_poseidon_bn254(17)
    cs = RC.case("S1")
    hip = HipBackend(prover=prover, hash_mode="bn128")
    key = G16.Key(cs.blob)
    proof, pubs, _ = G16.prove(key, *cs.set_lists(), hip, (0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321))
    assert len(pubs) >= 1 and GV.verify(key.vk, proof, pubs)
    assert G16.verify(key.vk, proof, pubs, hip) == ACCEPT
    assert G16.verify(key.vk, proof, pubs) == ACCEPT          # without a ctx
    bumped = [(pubs[0] + 1) % R] + pubs[1:]
    assert G16.verify(key.vk, proof, bumped, hip) == PAIRING and not GV.verify(key.vk, proof, bumped)
    assert G16.verify(key.vk, proof, [R] + pubs[1:], hip) == PUBLICS
    off = dict(proof, pi_c=(proof["pi_c"][0], (proof["pi_c"][1] + 1) % B.Q))
    assert G16.verify(key.vk, off, pubs, hip) == POINT
    assert G16.verify_batch(key.vk, [proof, off, proof], [pubs, pubs, bumped], hip) == [ACCEPT, POINT, PAIRING]


def test_engine_checks_its_final_proof():
    from eigen_zeth_amd.service.engine import Engine, EngineConfig
    from eigen_zeth_amd.service.server import default_backend_factory
    cfg = EngineConfig(air="chunk64", logn=12, chunks_per_block=1, n_queries=24, pow_bits=8, agg_queries=10, final_queries=6, groth16_seed="t", verify_final=True)
    eng = Engine(default_backend_factory(0), cfg)
    ch = eng.gen_batch_chunks("v", [7, 8], 12345, "evm")
    proofs = eng.gen_chunk_proofs("v", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    agg = eng.aggregate("v", proofs[0]["proof"], proofs[1]["proof"])
    js, pub = eng.final("v", agg, "BN128", "479881985774944702531460751064278034642760119942")
    assert '"pi_a"' in js and eng.stage_timings["final/v"]["groth16/verify"] > 0
