"""Service-level tests: the prover.v1 wire schema, the four-request sequence exactly as eigen-zeth's
ProverChannel drives it (src/prover/provider.rs:243-544), idempotent replays / resume across
connections, error convention, and the final-proof JSON grammar (src/settlement/ethereum/mod.rs:445-481).
The CPU runs use the oracle backend (BASELINE.json configs[0]: plumbing, no GPU); the -m gpu run
uses the HIP backend and must produce the same chunk proofs."""
import json
import os

import pytest

from eigen_zeth_amd.service import bn254, proto
from eigen_zeth_amd.service.client import ProverChannel, ProverClientError
from eigen_zeth_amd.service.engine import Engine, EngineConfig
from eigen_zeth_amd.service.server import ProverService, make_server
from eigen_zeth_amd.service.store import BatchStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_proof_like_eigen_zeth(js):
    """parse_proof (ethereum/mod.rs:445-474) through the product's mirror of the consumer (service/consumer.py, pinned on the reference's
    own vectors by tests/test_ref_proofs.py): the eight U256 in the order the contract receives them"""
    from eigen_zeth_amd.service import consumer
    return list(consumer.parse_proof(js).as_u256_tuple())


def parse_public_input_like_eigen_zeth(js):
    from eigen_zeth_amd.service import consumer
    return consumer.parse_public_input(js)[0]


def test_schema_matches_reference_proto_text():
    """the mirror's messages declare exactly the fields -- names and numbers -- of the reference's prover.proto, and the one rpc is
    bidirectionally streaming (tests/golden/ref_proto_schema.json, made from the schema by tests/golden/extract_ref_proto.py)"""
    with open(os.path.join(ROOT, "tests", "golden", "ref_proto_schema.json")) as f:
        ref = json.load(f)
    for mname, fields in proto.SCHEMA.items():
        assert mname in ref["messages"], mname
        assert {fname: num for (fname, num, *_rest) in fields} == ref["messages"][mname], mname
    assert ref["rpc"] == {"service": "ProverService", "method": "ProverStream", "request": "ProverRequest", "request_stream": True,
                          "response": "ProverResponse", "response_stream": True}
    assert proto.METHOD == "/prover.v1.%s/%s" % (ref["rpc"]["service"], ref["rpc"]["method"])


def test_schema_frozen_numbers():
    # survives without the reference: the numbers that are easy to get wrong (prover.proto:107-111,176-190)
    f = {n: num for (n, num, *_r) in proto.SCHEMA["ChunkProof"]}
    assert f == {"chunk_id": 1, "proof_key": 3, "proof": 2}
    assert min(num for (_n, num, *_r) in proto.SCHEMA["ProverStatus"]) == 2
    assert proto.METHOD == "/prover.v1.ProverService/ProverStream"
    r = proto.ProverResponse()
    r.gen_batch_proof.gen_batch_chunks.pre_state_root = b"\x01" * 32
    assert proto.ProverResponse.FromString(r.SerializeToString()).gen_batch_proof.gen_batch_chunks.pre_state_root == b"\x01" * 32


def test_reference_fixture_grammar():
    # the reference's own format fixtures (proof/proof.json, proof/public_input.json): shape only
    pts = parse_proof_like_eigen_zeth(open(os.path.join(ROOT, "tests/golden/ref_proof.json")).read())
    assert bn254.g1_on_curve((pts[0], pts[1])) and bn254.g1_on_curve((pts[6], pts[7]))
    assert bn254.g2_on_curve(((pts[2], pts[3]), (pts[4], pts[5])))
    assert parse_public_input_like_eigen_zeth(open(os.path.join(ROOT, "tests/golden/ref_public_input.json")).read()) < bn254.R


def _start(tmp_path, backend_factory, cfg=None):
    cfg = cfg or EngineConfig(air="wide8", logn=5, n_queries=3, fri_final_log=3, pow_bits=6)
    cfg.agg_queries, cfg.final_queries = 2, 2                         # small recursion layers: the CPU checker proves and verifies them
    cfg.crs_dir = str(tmp_path / "crs")
    engine = Engine(backend_factory, cfg)
    svc = ProverService(engine, BatchStore(str(tmp_path)))
    server, port = make_server(svc, port=0)
    server.start()
    return server, port, svc


@pytest.fixture()
def cpu_factory(tables):
    from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
    from cpu_wrap_backend import CpuWrapBackend
    return lambda hash_mode="gl": CpuWrapBackend(*tables, hash_mode=hash_mode,
                                                 bn_tables=bn254_poseidon_params(17) if hash_mode == "bn128" else None)


def _check_result(res, tables, block, svc=None):
    from eigen_zeth_amd.stark import air as AIR
    from oracle import stark_verify as V
    rc, mds = tables
    assert res["block_number"] == block
    assert len(res["pre_state_root"]) == 32 and len(res["post_state_root"]) == 32
    pts = parse_proof_like_eigen_zeth(res["proof"])
    assert bn254.g1_on_curve((pts[0], pts[1])) and bn254.g2_on_curve(((pts[2], pts[3]), (pts[4], pts[5])))
    pub = parse_public_input_like_eigen_zeth(res["public_input"])
    assert pub < bn254.R
    for p in res["chunk_proofs"]:
        pr = json.loads(p)
        assert V.verify(pr, AIR.get_air(pr["air"]).program(), rc, mds, V.expectation(svc.engine.stark_params(pr["params"]["logn"]).to_dict())
                        if svc is not None else V.expectation(pr["params"]))
    if svc is not None:   # the final proof is a Groth16 proof that verifies under the service's VK (pairing check)
        from oracle import groth16_verify as GV
        vk = json.loads(svc.engine.verifying_key_json())
        g1 = lambda d: (int(d["x"]), int(d["y"]))
        g2 = lambda d: ((int(d["x"][0]), int(d["x"][1])), (int(d["y"][0]), int(d["y"][1])))
        vkp = {"alpha1": g1(vk["alpha1"]), "beta2": g2(vk["beta2"]), "gamma2": g2(vk["gamma2"]), "delta2": g2(vk["delta2"]),
               "ic": [g1(p) for p in vk["ic"]]}
        proof = {"pi_a": (pts[0], pts[1]), "pi_b": ((pts[2], pts[3]), (pts[4], pts[5])), "pi_c": (pts[6], pts[7])}
        assert GV.verify(vkp, proof, [pub])
        assert not GV.verify(vkp, proof, [(pub + 1) % bn254.R])
        meta = json.loads(res["proof"])
        assert "final-stark-verifier (stage B-2" in meta["circuit"] and len(meta["zeta"]) == 3
        # ... and it names (by digest) a final STARK in BN128-hash mode that the independent verifier accepts
        import hashlib
        from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
        fs = [v for v in svc.engine.final_starks.values() if hashlib.sha256(v.encode()).hexdigest() == json.loads(res["proof"])["final_stark_sha256"]]
        assert len(fs) == 1
        fsp = json.loads(fs[0])
        assert fsp["params"]["hash"] == "bn128" and len(fsp["roots"]["trace"]) == 1
        # stage B-2 (round 6): the wrap's one public input commits to PUBLIC data only -- the statement's public inputs (through their commitment), the
        # aggregator address of the request, zeta and the statement's sparse fixed columns at zeta: the checker recomputes it WITHOUT the final STARK's
        # openings, evaluations or roots (oracle/wrap_verify.py: public_input_b2 reads the statement, its public inputs and the proof text's zeta)
        from oracle import wrap_verify as WV
        from eigen_zeth_amd.service.client import DEFAULT_AGGREGATOR_ADDR
        fs_id = [k for k, v in svc.engine.final_starks.items() if v == fs[0]][0]
        agg_stark = json.loads(res["aggregated"])["stark"]
        fparams = svc.engine.final_stark_params(agg_stark).to_dict()
        assert pub == WV.public_input_b2(svc.engine.final_programs[fs_id], fparams, fsp["root32"], fsp["shift"], fsp["publics"], int(DEFAULT_AGGREGATOR_ADDR),
                                         [int(v) for v in meta["zeta"]], bn254_poseidon_params(17))
        assert pub != WV.public_input_b2(svc.engine.final_programs[fs_id], fparams, fsp["root32"], fsp["shift"], fsp["publics"], int(DEFAULT_AGGREGATOR_ADDR) + 1,
                                         [int(v) for v in meta["zeta"]], bn254_poseidon_params(17))
        # the recursion layers prove what they name.  (1) the aggregated proof: both chunk-proof headers verify (transcript,
        # out-of-domain identity, final layer), the outer STARK's publics are their roots and transcript-derived indices, and
        # the outer STARK verifies under the Merkle-verifier AIR of that shape
        from eigen_zeth_amd.stark import verifier_air as VA
        from oracle import aggregate_verify as AV
        agg = json.loads(res["aggregated"])
        assert agg["kind"] == "aggregated" and "standin" not in res["aggregated"]
        inner_air = AIR.get_air(agg["inner"][0]["air"])
        sh = VA.Shape.from_dict(agg["shape"])
        vair = VA.verifier_air(sh, rc, mds)
        assert vair.digest() == agg["verifier_air_digest"] and sh.n_slots() == agg["slots"]
        inner_exp = V.expectation(svc.engine.stark_params(sh.logn).to_dict())
        outer_exp = V.expectation(VA.aggregation_params(sh, svc.engine.cfg.agg_queries, svc.engine.cfg.fri_logf, svc.engine.cfg.fri_final_log).to_dict())
        assert AV.verify(agg, inner_air.program(), vair.program(), rc, mds, inner_exp, outer_exp, sh.n_slots())
        # (2) the final STARK (BN128-hash mode): the same verifier AIR over the aggregated proof's STARK -- its publics are that
        # STARK's roots and query indices, and the independent verifier accepts it
        fsh = VA.Shape.of_proof(agg["stark"], 1)
        fair = VA.verifier_air(fsh, rc, mds)
        assert fsp["air_digest"] == fair.digest()
        assert [int(v) for v in fsp["publics"]][:fsh.merkle_pubs()] == VA.expected_publics(fsh, [agg["stark"]])
        assert V.verify(fsp, fair.program(), rc, mds, V.expectation(svc.engine.final_stark_params(agg["stark"]).to_dict()),
                        bn254_poseidon_params(17))
        # ... and as a recursion layer: the aggregated proof's STARK without its paths + the final STARK = that STARK verifies
        # (its arithmetic natively, its transcript read off the final STARK's public inputs, all hashing in the final STARK)
        assert all("queries" not in h for h in agg["inner"]) and '"values"' not in res["aggregated"].split('"stark":')[0]   # headers only
        hdr = {k: v for k, v in agg["stark"].items() if k != "queries"}
        assert AV.verify({"inner": [hdr], "stark": fsp}, vair.program(), fair.program(), rc, mds, outer_exp,
                         V.expectation(svc.engine.final_stark_params(agg["stark"]).to_dict()), fsh.n_slots(), bn254_poseidon_params(17))
    # ProofResult as eigen-zeth stores it (src/db/mod.rs:63-71): json with 32-number arrays
    stored = json.dumps({k: res[k] for k in ("block_number", "proof", "public_input", "pre_state_root", "post_state_root")})
    assert len(json.loads(stored)["pre_state_root"]) == 32


def test_empty_block_batch_round_trip_cpu(tmp_path, cpu_factory, tables):
    server, port, svc = _start(tmp_path, cpu_factory)
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        res = ch.execute(1)   # genesis+1 empty block (BASELINE configs[0])
        assert ch.trace == [("gen_batch_proof", "gen_batch_proof")] * 2 + [("gen_aggregated_proof", "gen_aggregated_proof"),
                                                                          ("gen_final_proof", "gen_final_proof")]
        _check_result(res, tables, 1, svc)
        st = ch.get_status()
        assert st.status == proto.STATUS_IDLE and st.prover_status.version_server.startswith("zeth-prover")
        # consecutive blocks chain their state roots
        res2 = ch.execute(2)
        assert res2["pre_state_root"] == res["post_state_root"]
        ch.close()
    finally:
        server.stop(0)


def test_replay_and_resume_are_idempotent(tmp_path, cpu_factory):
    server, port, svc = _start(tmp_path, cpu_factory)
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        a = ch.execute(7, batch_id="b-7")
        calls = dict(n=0)
        orig = svc.engine.gen_chunk_proofs
        svc.engine.gen_chunk_proofs = lambda *x: (calls.__setitem__("n", calls["n"] + 1), orig(*x))[1]
        b = ch.execute(7, batch_id="b-7")          # verbatim replay on the same stream
        ch.close()
        ch2 = ProverChannel("127.0.0.1:%d" % port)  # a new connection (client restarted, PROVE_STEP_RECORD resume)
        c = ch2.execute(7, batch_id="b-7")
        ch2.close()
        assert a == b == c and calls["n"] == 0
    finally:
        server.stop(0)
    # a new server process over the same state directory still answers from the store
    server, port, svc = _start(tmp_path, cpu_factory)
    try:
        svc.engine.gen_chunk_proofs = lambda *x: (_ for _ in ()).throw(AssertionError("recomputed"))
        ch = ProverChannel("127.0.0.1:%d" % port)
        assert ch.execute(7, batch_id="b-7") == a
        ch.close()
    finally:
        server.stop(0)


def test_error_convention(tmp_path, cpu_factory):
    server, port, svc = _start(tmp_path, cpu_factory)
    try:
        ch = ProverChannel("127.0.0.1:%d" % port, program_name="wasm")
        with pytest.raises(ProverClientError):
            ch.execute(3, max_retries=2)
        assert ch.trace == [("gen_batch_proof", "gen_batch_proof")] * 2   # retried, same response type
        ch.close()
        ch = ProverChannel("127.0.0.1:%d" % port, curve="BLS12381")
        with pytest.raises(ProverClientError):
            ch.execute(3, max_retries=1)
        ch.close()
        # malformed: chunk_count not matching batch_data -> COMPLETED_ERROR and no batch_proof_result
        ch = ProverChannel("127.0.0.1:%d" % port)
        req = proto.ProverRequest(id="x")
        g = req.gen_batch_proof.gen_chunk_proof
        g.batch_id, g.task_id, g.chunk_count, g.batch_data = "bad", "0000000001", 2, json.dumps({"chunks": []})
        r = ch._call(req).gen_batch_proof.gen_chunk_proof
        assert r.result_code == proto.COMPLETED_ERROR and not r.HasField("batch_proof_result") and r.error_message
        ch.close()
    finally:
        server.stop(0)


def test_product_service_needs_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eigen_zeth_amd.native import ZpError
    from eigen_zeth_amd.service.server import default_backend_factory
    with pytest.raises(ZpError):
        Engine(default_backend_factory()).be


@pytest.mark.gpu
def test_round_trip_gpu_matches_cpu(tmp_path, cpu_factory, tables):
    from eigen_zeth_amd.service.server import default_backend_factory
    cfg = EngineConfig(air="chunk64", logn=12, n_queries=8, pow_bits=12)
    server, port, svc = _start(tmp_path / "gpu", default_backend_factory(), cfg)
    server2, port2, svc2 = _start(tmp_path / "cpu", cpu_factory, cfg)
    try:
        ch, ch2 = ProverChannel("127.0.0.1:%d" % port), ProverChannel("127.0.0.1:%d" % port2)
        g, c = ch.execute(5, batch_id="same"), ch2.execute(5, batch_id="same")
        _check_result(g, tables, 5, svc)
        _check_result(c, tables, 5, svc2)
        # identical chunk STARKs / public_input / roots from the MI355X and from the CPU restatement; the final Groth16
        # proofs carry fresh blinding (r, s) per proof, so they differ as group elements and both verify (above)
        assert {k: v for k, v in g.items() if k != "proof"} == {k: v for k, v in c.items() if k != "proof"}
        assert g["proof"] != c["proof"]
        # the final STARKs (BN128-hash mode) behind the two wraps are the same bytes
        assert json.loads(g["proof"])["final_stark_sha256"] == json.loads(c["proof"])["final_stark_sha256"]
        ch.close(); ch2.close()
    finally:
        server.stop(0); server2.stop(0)


def test_block_input_fetcher_with_stub_node(tmp_path, cpu_factory):
    """with an L2 JSON-RPC endpoint configured, state roots and chunk counts come from the block"""
    import http.server
    import threading

    blocks = {n: {"number": hex(n), "hash": "0x" + "%064x" % (n + 7), "stateRoot": "0x" + "%064x" % (1000 + n),
                  "transactions": ["0x" + "%064x" % i for i in range(3 if n == 5 else 0)]} for n in range(0, 8)}

    class H(http.server.BaseHTTPRequestHandler):
        def do_POST(self):
            q = json.loads(self.rfile.read(int(self.headers["Content-Length"])))
            assert q["method"] == "eth_getBlockByNumber"
            body = json.dumps({"jsonrpc": "2.0", "id": q["id"], "result": blocks.get(int(q["params"][0], 16))}).encode()
            self.send_response(200); self.send_header("Content-Type", "application/json"); self.end_headers(); self.wfile.write(body)

        def log_message(self, *a):
            pass

    httpd = http.server.HTTPServer(("127.0.0.1", 0), H)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    cfg = EngineConfig(air="fib", logn=5, n_queries=4, fri_final_log=3, pow_bits=4, l2_addr="http://127.0.0.1:%d" % httpd.server_port, txs_per_chunk=2)
    server, port, svc = _start(tmp_path, cpu_factory, cfg)
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        res = ch.execute(5)
        assert bytes(res["pre_state_root"]) == bytes.fromhex("%064x" % 1004) and bytes(res["post_state_root"]) == bytes.fromhex("%064x" % 1005)
        assert len(res["chunk_proofs"]) == 2           # 3 transactions, 2 per chunk
        # every chunk proof is bound to ITS block: the leading public inputs are the limbs of the block statement (roots, block
        # hash, transaction digest as the node reports them -- recomputed here from the stub's data by the checker), the
        # STARK verifies with them, and the same proof is rejected as a proof for the next block
        from oracle import statement as ST
        from oracle import stark_verify as V
        from eigen_zeth_amd.stark import air as AIR
        import numpy as np
        from eigen_zeth_amd.poseidon_constants import default_round_constants, default_mds
        rcm = (np.array(default_round_constants(), dtype=np.uint64), np.array(default_mds(), dtype=np.uint64))

        def ctx(n):
            return dict(pre_root=bytes.fromhex("%064x" % (1000 + n - 1)), post_root=bytes.fromhex("%064x" % (1000 + n)),
                        block_hash=bytes.fromhex(blocks[n]["hash"][2:]), txd=ST.tx_digest(blocks[n]["transactions"]))
        exp = V.expectation(svc.engine.stark_params(5).to_dict())
        for k, cp in enumerate(res["chunk_proofs"]):
            pr = json.loads(cp)
            assert V.verify(pr, AIR.get_air("fib").program(), rcm[0], rcm[1], exp)
            assert ST.bound_to(pr, 12345, 5, k, 2, n=2, **ctx(5))
            assert not ST.bound_to(pr, 12345, 6, k, 2, n=2, **ctx(6))        # a proof for block 5 is not a proof for block 6
            assert not ST.bound_to(pr, 12345, 5, 1 - k, 2, n=2, **ctx(5))    # nor for the other chunk of its block
            forged = dict(pr, publics=ST.limbs(12345, 6, k, 2, n=2, **ctx(6)) + pr["publics"][2:])
            with pytest.raises(V.Reject):                                    # relabelling the publics breaks the transcript
                V.verify(forged, AIR.get_air("fib").program(), rcm[0], rcm[1], exp)
        assert len(ch.execute(6)["chunk_proofs"]) == 1  # empty block still gets one chunk
        with pytest.raises(ProverClientError):
            ch.execute(99, max_retries=1)               # unknown block -> COMPLETED_ERROR
        ch.close()
    finally:
        server.stop(0); httpd.shutdown()


def test_metrics_endpoint_counts_requests_and_stage_time(tmp_path, cpu_factory):
    """Prometheus text on /metrics with request counters, per-stage seconds and the HBM rate gauge"""
    import urllib.request
    from eigen_zeth_amd.service.metrics import Metrics
    cfg = EngineConfig(air="chunk16", logn=5, n_queries=2, fri_final_log=3, pow_bits=4, agg_queries=2, final_queries=2)
    cfg.crs_dir = str(tmp_path / "crs")
    m = Metrics()
    httpd = m.serve(0)
    svc = ProverService(Engine(cpu_factory, cfg), BatchStore(str(tmp_path)), m)
    server, port = make_server(svc, port=0)
    server.start()
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        ch.execute(3)
        ch.close()
        txt = urllib.request.urlopen("http://127.0.0.1:%d/metrics" % httpd.server_address[1]).read().decode()
        assert 'zeth_prover_requests_total{type="gen_chunk_proof",outcome="ok"} 1' in txt
        assert 'zeth_prover_requests_total{type="gen_final_proof",outcome="ok"} 1' in txt
        assert "zeth_prover_chunk_proofs_total 1" in txt
        assert 'zeth_prover_stage_seconds_count{stage="grand-product+lde+merkle(stage2)"} 1' in txt
        assert 'zeth_prover_stage_seconds_count{stage="groth16"} 1' in txt
        assert 'zeth_prover_stage_hbm_gbps{stage="lde+merkle(trace)"}' in txt
        with pytest.raises(Exception):
            urllib.request.urlopen("http://127.0.0.1:%d/other" % httpd.server_address[1])
    finally:
        server.stop(0); httpd.shutdown()


def test_chunk_proofs_identical_across_streams_and_devices(tmp_path, cpu_factory):
    """the engine proves chunks on several backends in parallel (streams of one GPU, or one factory per GPU):
    the batch result must not depend on how many there are"""
    def run(factories, streams):
        cfg = EngineConfig(air="chunk16", logn=6, n_queries=4, fri_final_log=3, pow_bits=4, chunks_per_block=1, prover_streams=streams,
                           witness_threads=3)
        cfg.crs_dir = str(tmp_path / "crs")
        eng = Engine(factories, cfg)
        ch = eng.gen_batch_chunks("b", [3, 4, 5, 6, 7], 12345, "evm")
        return eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    one = run(cpu_factory, 1)
    assert [p["chunk_id"] for p in one] == [0, 1, 2, 3, 4]
    assert run(cpu_factory, 3) == one
    assert run([cpu_factory, cpu_factory], 2) == one


def test_two_concurrent_streams_replaying_one_request(tmp_path, cpu_factory):
    """A reconnecting client replays GenChunkProof on a new stream while the old handler is still proving
    (src/prover/provider.rs:671-700).  The service must answer both with the same proofs, compute them once, and never
    drive one backend from two threads."""
    import threading
    from eigen_zeth_amd.service import proto
    cfg = EngineConfig(air="chunk16", logn=7, n_queries=4, fri_final_log=3, pow_bits=4, chunks_per_block=3, prover_streams=2)
    server, port, svc = _start(tmp_path, cpu_factory, cfg)
    calls, inside, overlap = [], [0], [0]
    real = svc.engine._gen_chunk_proofs

    def counted(*a):
        inside[0] += 1
        overlap[0] = max(overlap[0], inside[0])
        try:
            calls.append(a[1])
            return real(*a)
        finally:
            inside[0] -= 1
    svc.engine._gen_chunk_proofs = counted
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        q = proto.ProverRequest(id="1")
        g = q.gen_batch_proof.gen_batch_chunks
        g.batch_id, g.chain_id, g.program_name = "dup", 12345, "evm"
        g.batch.block_number.append(9)
        r = ch._call(q).gen_batch_proof.gen_batch_chunks
        assert r.result_code == proto.COMPLETED_OK and r.chunk_count == 3
        out = [None, None]

        def go(i):
            c = ProverChannel("127.0.0.1:%d" % port)
            q = proto.ProverRequest(id="r%d" % i)       # the replay carries a new request id, same batch_id
            g = q.gen_batch_proof.gen_chunk_proof
            g.batch_id, g.task_id, g.chunk_count, g.chain_id, g.program_name, g.batch_data = "dup", r.task_id, r.chunk_count, 12345, "evm", r.batch_data
            out[i] = c._call(q).gen_batch_proof.gen_chunk_proof
            c.close()
        ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        ch.close()
        a, b = out
        assert a.result_code == proto.COMPLETED_OK and b.result_code == proto.COMPLETED_OK
        pa = [(p.chunk_id, p.proof) for p in a.batch_proof_result.chunk_proofs]
        assert pa == [(p.chunk_id, p.proof) for p in b.batch_proof_result.chunk_proofs] and len(pa) == 3
        assert len(calls) == 1 and overlap[0] == 1      # computed once; the replay waited and read the stored result
        # the engine itself serialises direct callers too
        e2 = [None, None]

        def direct(i):
            e2[i] = svc.engine.gen_chunk_proofs("x%d" % i, r.task_id, r.chunk_count, r.batch_data)
        ts = [threading.Thread(target=direct, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert e2[0] == e2[1] and overlap[0] == 1
    finally:
        server.stop(0)


def test_get_status_answers_while_replays_queue_behind_a_running_proof(tmp_path, cpu_factory):
    """Six streams replay one slow GenChunkProof (a client that keeps reconnecting, src/prover/provider.rs:671-700); a
    GetStatus on yet another stream must be answered at once -- COMPUTING -- and must still say COMPUTING after the first
    replays have been answered while others are pending (one handler finishing does not clear another one's entry)."""
    import threading
    import time
    from eigen_zeth_amd.service import proto
    cfg = EngineConfig(air="fib", logn=5, n_queries=4, fri_final_log=3, pow_bits=4)
    server, port, svc = _start(tmp_path, cpu_factory, cfg)
    real = svc.engine._gen_chunk_proofs
    started, release = threading.Event(), threading.Event()

    def slow(*a):
        started.set()
        release.wait(30)
        return real(*a)
    svc.engine._gen_chunk_proofs = slow
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        q = proto.ProverRequest(id="1")
        g = q.gen_batch_proof.gen_batch_chunks
        g.batch_id, g.chain_id, g.program_name = "slow", 12345, "evm"
        g.batch.block_number.append(4)
        r = ch._call(q).gen_batch_proof.gen_batch_chunks
        out = [None] * 6

        def go(i):
            c = ProverChannel("127.0.0.1:%d" % port)
            q = proto.ProverRequest(id="same-id")
            g = q.gen_batch_proof.gen_chunk_proof
            g.batch_id, g.task_id, g.chunk_count, g.chain_id, g.program_name, g.batch_data = "slow", r.task_id, r.chunk_count, 12345, "evm", r.batch_data
            out[i] = c._call(q).gen_batch_proof.gen_chunk_proof
            c.close()
        ts = [threading.Thread(target=go, args=(i,)) for i in range(6)]
        for t in ts:
            t.start()
        assert started.wait(20)
        time.sleep(0.3)                      # let the other five reach their batch lock
        t0 = time.time()
        st = ch.get_status()
        assert time.time() - t0 < 5 and st.status == proto.STATUS_COMPUTING
        release.set()
        for t in ts:
            t.join()
        assert all(o.result_code == proto.COMPLETED_OK for o in out)
        assert len({tuple(p.proof for p in o.batch_proof_result.chunk_proofs) for o in out}) == 1
        st = ch.get_status()
        assert st.status == proto.STATUS_IDLE and st.prover_status.last_computed_request_id == "same-id"
        ch.close()
    finally:
        release.set()
        server.stop(0)


def test_hybrid_witness_selection_gives_the_same_batch(tmp_path, cpu_factory):
    """EngineConfig.witness = "device": the first witness_threads chunks (in processing order) come from the host generator, the others are
    filled from checkpoints of ONE walk per GPU -- here on a stand-in backend whose "device" fill is the host generator itself, so that the
    control flow (which chunk takes which path, the index of a chunk in its GPU's checkpoint buffer, the fall-back when the fill fails)
    runs without a GPU.  The batch must not depend on the path a witness took."""
    from eigen_zeth_amd import native
    calls = {"ckpt": [], "fill": [], "fail": 0}

    class Ckpt:
        def __init__(self, seeds, binds):
            self.seeds, self.binds = list(seeds), [list(b) for b in binds]

        def free(self):
            pass

    def factory(fail_fills=False):
        def make(hash_mode="gl"):
            be = cpu_factory(hash_mode)

            def synth_checkpoints(air, logn, seeds, binds):
                calls["ckpt"].append(len(seeds))
                return Ckpt(seeds, binds)

            def synth_trace_device(air, logn, seed, bind, ck, index):
                assert ck.seeds[index] == seed and ck.binds[index] == list(bind or [])      # the chunk's own slot of the buffer
                if fail_fills:
                    calls["fail"] += 1
                    raise native.ZpError(-3, "no device memory (stand-in)")
                calls["fill"].append(seed)
                return native.synth_trace(air.trace_kind, logn, air.width, seed, bind=bind)

            be.synth_checkpoints, be.synth_trace_device = synth_checkpoints, synth_trace_device
            return be
        return make

    def run(fac, witness):
        cfg = EngineConfig(air="chunk16", logn=6, n_queries=4, fri_final_log=3, pow_bits=4, chunks_per_block=1, prover_streams=2, witness_threads=2,
                           witness=witness)
        cfg.crs_dir = str(tmp_path / "crs")
        eng = Engine(fac, cfg)
        ch = eng.gen_batch_chunks("b", [3, 4, 5, 6, 7, 8, 9], 12345, "evm")
        return eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    host = run(cpu_factory, "host")
    dev = run(factory(), "device")
    assert dev == host
    assert calls["ckpt"] == [5] and len(calls["fill"]) == 5            # 7 chunks, 2 witness threads: two from the host, five filled
    calls["ckpt"].clear()
    assert run([factory(), factory()], "device") == host                # two GPUs: one walk each over the chunks it proves
    assert sorted(calls["ckpt"]) == [2, 3]
    assert run(factory(fail_fills=True), "device") == host and calls["fail"] == 5      # every fill fails: the host generator takes over
