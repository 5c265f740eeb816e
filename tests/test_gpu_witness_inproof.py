"""The GENERATED witness-check kernels (stark/air.py: emit_witness_source -> `<symbol>_witness`, run by csrc/witness_check.hip under the knob
"witness_kernel") and the check INSIDE the one-call provers (knob "prove_check", ZP_ERR_WITNESS, zp_stark_prove_witness_report).

Every expectation is the checker's own row walk (tests/witness_cases.py: oracle_report) -- exact integers, never the interpreter kernel's output; the
interpreter form and the host path are compared with the same expectation on the same buffer.  Sizes: N = 2 (logn 1), less than a wave (5), one wave
(6), one workgroup (8), two (9), sixteen (12: the exact counts).  Two cases cannot be built as the sizes are listed and are written down here:
`periodic` has a fixed column of period 8, so on 2 rows the statement does not exist -- both forms must REFUSE it (ZP_ERR_ARG), and its smallest
size, logn 3, is checked instead; the flip at (W/2, N/2 + 1) is taken mod N, which on 2 rows is row 0.

In the proof the stage-2 challenge is the transcript's: the expectation's challenge is recorded from the CPU restatement (stark/prover.py over
oracle.stark_cpu.CpuBackend on the same false trace, stopped at commit_stage2)."""
import json

import numpy as np
import pytest

import witness_cases as WC
from test_witness_check_host import host_check, raw_check
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import prover as PR

pytestmark = pytest.mark.gpu

P = WC.P
NONE = WC.NONE
GEN, INTERP = "witness_program_gen", "witness_program"


@pytest.fixture(scope="module")
def hip(prover):
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    be = HipBackend(prover=prover)
    yield be
    prover.set_tuning("witness_kernel", 1)
    prover.set_tuning("prove_check", 0)
    prover.set_profiling(False)


def register(hip, air):
    hip.p.set_air_kernel_witness(air.program(), hip._airlib_witness(air))


def stages_of(prover, call):
    prover.set_profiling(True)
    prover.stage_timings()
    try:
        out = call()
        return out, [e["stage"] for e in prover.stage_timings()]
    finally:
        prover.set_profiling(False)


def both_forms(prover, blob, trace, pubs, logn, chal=None):
    """(report, counts, first rows) through the generated kernel; the interpreter form on the SAME buffer must give the same words, the stage
    clock must show which form ran, and the trace must come back unchanged"""
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    d = prover.upload(tr)
    try:
        got = {}
        for knob, ran, other in ((1, GEN, INTERP), (0, INTERP, GEN)):
            prover.set_tuning("witness_kernel", knob)
            (rc, rep, counts, first), stages = stages_of(prover, lambda: raw_check(prover.ctx, blob, d.ptr, tr.size, pubs, logn, chal))
            assert rc == 0, prover.lib.zp_last_error(prover.ctx)
            if rep[0] != WC.NONCANONICAL:
                assert ran in stages and other not in stages, (knob, stages)
            got[knob] = (rep, counts, first)
        assert got[0] == got[1]
        assert (prover.download(d, tr.shape) == tr).all()
    finally:
        prover.set_tuning("witness_kernel", 1)
        d.free()
    return got[1]


def agree(prover, blob, trace, pubs, logn, chal=None):
    want = WC.oracle_report(blob, trace, pubs, logn, chal)
    assert host_check(blob, trace, pubs, logn, chal) == want
    assert both_forms(prover, blob, trace, pubs, logn, chal) == want
    return want


# ---------------------------------------------------------------------------------------------- the generated kernel against the oracle
@pytest.mark.parametrize("logn", [1, 5, 6, 8, 9])
@pytest.mark.parametrize("name", WC.SATISFIED_AIRS)
def test_generated_kernel_honest_and_flipped(prover, hip, name, logn):
    if name == "periodic" and logn == 1:
        from eigen_zeth_amd.stark import air as AIR
        air = AIR.periodic_air(3)
        register(hip, air)
        blob = np.ascontiguousarray(air.program(), dtype=np.uint64)
        d = prover.upload(np.zeros((air.width, 2), dtype=np.uint64))
        try:
            for knob in (1, 0):                       # a period of 8 on 2 rows: no such statement, whichever form would run
                prover.set_tuning("witness_kernel", knob)
                assert raw_check(prover.ctx, blob, d.ptr, air.width * 2, [1, 2], 1)[0] == -1
        finally:
            prover.set_tuning("witness_kernel", 1)
            d.free()
        logn = 3
    N = 1 << logn
    air, blob, trace, pubs = WC.honest_case(name, logn)
    register(hip, air)
    K = int(blob[8])
    for chal in ([None, WC.EXPLICIT_CHALLENGE] if air.stage2 else [None]):
        assert agree(prover, blob, trace, pubs, logn, chal) == ([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K)
    for col, row in [(0, 0), (0, N - 1), (air.width - 1, N - 1), (air.width // 2, (N // 2 + 1) % N)]:
        assert agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)[0][0] == WC.VIOLATED, (col, row)


def test_flips_at_wave_and_workgroup_seams(prover, hip):
    logn = 9
    for name in ("fib", "chunk16"):
        air, blob, trace, pubs = WC.honest_case(name, logn)
        register(hip, air)
        for row in (63, 64, 255, 256):
            for col in (0, air.width - 1):
                want = agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)
                assert want[0][0] == WC.VIOLATED and row - 1 <= want[0][1] <= row


@pytest.mark.parametrize("logn", [6, 9])
def test_broken_stage2_arguments(prover, hip, logn):
    N = 1 << logn
    for make, name in ((WC.broken_perm, "perm"), (WC.broken_lookup, "chunk16")):
        register(hip, WC.honest_case(name, logn)[0])
        blob, bad, pubs = make(logn)
        for chal in (None, WC.EXPLICIT_CHALLENGE):
            want = agree(prover, blob, bad, pubs, logn, chal)
            assert want[0][0] == WC.VIOLATED and want[0][1] == N - 1


@pytest.mark.parametrize("logn", [12, 5])
def test_exact_counts_on_a_random_trace(prover, hip, logn):
    """chunk16's program over a seeded random canonical trace: nearly every row violates nearly every constraint; counts are the oracle's integers --
    the ballot sum over 64 waves (logn 12) and the dead-lane mask (logn 5: 32 live lanes of 256)"""
    air, blob, _, _ = WC.honest_case("chunk16", logn)
    register(hip, air)
    trace, pubs = WC.random_inputs(dict(width=air.width, n_pub=air.n_pub), logn, 7001 + logn)
    want = agree(prover, blob, trace, pubs, logn)
    N = 1 << logn
    # (the stage-2 columns are made from the trace, so their own constraints hold by construction away from the wrap-around row: the wide mix, the
    # Fibonacci pair, c = r^2, d = fa r + fb and the range step are the ones violated at nearly every row)
    assert want[0][0] == WC.VIOLATED and want[0][3] == sum(want[1]) and sum(c >= N - 1 for c in want[1]) >= 8


def verifier_air():
    """the AIR object behind WC.verifier_air_case() (which keeps only its blob): the same steps, the same program"""
    from eigen_zeth_amd.poseidon_constants import default_mds, default_round_constants
    from eigen_zeth_amd.stark import air as AIR, verifier_air as VA
    from oracle.stark_cpu import CpuBackend
    rc, mds = np.array(default_round_constants(), dtype=np.uint64), np.array(default_mds(), dtype=np.uint64)
    air = AIR.get_air("fib")
    tr, pub = native.synth_trace(air.trace_kind, 5, air.width, 9)
    proof = json.loads(PR.proof_to_json(PR.prove(air, tr, pub, PR.StarkParams(5, 1, 2, 3, 3, pow_bits=0), CpuBackend(rc, mds))))
    return VA.verifier_air(VA.Shape.of_proof(proof, 1), rc, mds)


def test_recursion_statement_through_compile_air_kernel(prover, hip):
    """a verifier AIR: ~100 sparse fixed columns with public-input entries, their offsets and masks baked into the kernel"""
    blob, trace, pubs, logn = WC.verifier_air_case()
    vair = verifier_air()
    assert (np.asarray(vair.program(), dtype=np.uint64) == blob).all()
    assert hip.compile_air_kernel(vair)
    K = int(blob[8])
    assert agree(prover, blob, trace, pubs, logn) == ([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K)
    for col, row in ((30, 77), (0, 0), (46, (1 << logn) - 1), (12, 2048)):
        assert agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)[0][0] == WC.VIOLATED


# ---------------------------------------------------------------------------------------------- the check in the proof
LOGN = 8
PARAMS = PR.StarkParams(LOGN, 1, 3, 3, 6, pow_bits=4)          # test_check_then_prove_on_the_same_buffer's
ARGS = (PARAMS.logn, PARAMS.logb, PARAMS.fri_logf, PARAMS.fri_final_log, PARAMS.n_queries, PARAMS.pow_bits)


def recorded_challenge(air, trace, pubs, tables, params=PARAMS):
    """the stage-2 challenge of the CPU restatement of the protocol on this trace (None: the AIR has no stage 2)"""
    from oracle.stark_cpu import CpuBackend

    class Reached(Exception):
        pass

    class Recorder(CpuBackend):
        def commit_stage2(self, air, c1, chal, *a, **kw):
            self.chal = [int(v) for v in chal]
            raise Reached
    be = Recorder(*tables)
    if not air.stage2:
        return None
    with pytest.raises(Reached):
        PR.prove(air, np.ascontiguousarray(trace), pubs, params, be)
    return be.chal


def raw_prove(prover, air, blob, d, pubs, bn=False):
    """the C call itself: (rc, text or None, zp_last_error)"""
    import ctypes as C
    pb = np.array([int(v) for v in pubs] + [0], dtype=np.uint64)
    out, n = C.c_void_p(), C.c_size_t(0)
    head = (prover.ctx, air.name.encode(), blob.ctypes.data, blob.size, d.ptr, blob[1] << LOGN, pb.ctypes.data, len(pubs))
    if bn:
        rc = prover.lib.zp_stark_prove_bn128(*head, *ARGS[:5], C.byref(out), C.byref(n))
    else:
        rc = prover.lib.zp_stark_prove(*head, *ARGS, C.byref(out), C.byref(n))
    if rc != 0:
        assert out.value is None and n.value == 0
        return rc, None, (prover.lib.zp_last_error(prover.ctx) or b"").decode()
    try:
        return rc, C.string_at(out.value, n.value).decode(), ""
    finally:
        prover.lib.zp_free_buffer(out)


def raw_report(prover, K):
    import ctypes as C
    rep, chal, counts, first = (np.full(n, 0xA5A5A5A5, dtype=np.uint64) for n in (8, 3, max(K, 1), max(K, 1)))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = prover.lib.zp_stark_prove_witness_report(prover.ctx, p(rep), p(chal), p(counts), p(first), K)
    return rc, [int(v) for v in rep], [int(v) for v in chal], [int(v) for v in counts[:K]], [int(v) for v in first[:K]]


def test_report_before_any_checked_proof():
    p = native.Prover(0)
    try:
        rc, rep, _, _, _ = raw_report(p, 5)
        assert rc == -1 and rep == [0xA5A5A5A5] * 8
        air, blob, trace, pubs = WC.honest_case("fib", LOGN)
        d = p.upload(np.ascontiguousarray(trace))
        assert raw_prove(p, air, blob, d, pubs)[0] == 0                     # an unchecked proof leaves no report
        assert raw_report(p, 5)[0] == -1
        p.set_tuning("prove_check", 1)
        assert raw_prove(p, air, blob, d, pubs)[0] == 0
        K = int(blob[8])
        assert raw_report(p, K) == (0, [WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0, 0, 0], [0] * K, [NONE] * K)
        assert raw_report(p, K + 1)[0] == -1 and raw_report(p, K - 1)[0] == -1
        for bad in (2, -1):
            with pytest.raises(native.ZpError):
                p.set_tuning("prove_check", bad)
            with pytest.raises(native.ZpError):
                p.set_tuning("witness_kernel", bad)
        d.free()
    finally:
        p.close()


@pytest.mark.parametrize("name", ["fib", "perm", "chunk16", "periodic"])
def test_checked_proofs(prover, hip, tables, name):
    air, blob, trace, pubs = WC.honest_case(name, LOGN)
    register(hip, air)
    K, N = int(blob[8]), 1 << LOGN
    tr = np.ascontiguousarray(trace)
    d, d_bad = prover.upload(tr), prover.alloc(tr.size)
    try:
        prover.set_tuning("prove_check", 0)
        rc, plain, _ = raw_prove(prover, air, blob, d, pubs)
        assert rc == 0
        honest_chal = recorded_challenge(air, tr, pubs, tables) or [0, 0, 0]

        def honest_again():
            for knob, ran in ((1, GEN), (0, INTERP)):
                prover.set_tuning("witness_kernel", knob)
                (rc, text, err), stages = stages_of(prover, lambda: raw_prove(prover, air, blob, d, pubs))
                assert rc == 0 and text == plain, err
                assert ran in stages and "witness_canonical" in stages
                assert raw_report(prover, K) == (0, [WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], honest_chal, [0] * K, [NONE] * K)
            prover.set_tuning("witness_kernel", 1)
            assert (prover.download(d, tr.shape) == tr).all()
        prover.set_tuning("prove_check", 1)
        honest_again()
        bads = [WC.flipped(trace, air.width // 2, N // 2 + 1), WC.flipped(trace, 0, 0)]
        if name == "perm":
            bads.append(WC.broken_perm(LOGN)[1])
        if name == "chunk16":
            bads.append(WC.broken_lookup(LOGN)[1])
        for bad in bads:
            bad = np.ascontiguousarray(bad)
            chal = recorded_challenge(air, bad, pubs, tables)
            want = WC.oracle_report(blob, bad, pubs, LOGN, chal)
            assert want[0][0] == WC.VIOLATED
            prover.h2d(d_bad, bad)
            for knob in (1, 0):
                prover.set_tuning("witness_kernel", knob)
                rc, text, err = raw_prove(prover, air, blob, d_bad, pubs)
                assert rc == native.ZP_ERR_WITNESS == -7 and text is None
                assert "constraint %d at row %d" % (want[0][2], want[0][1]) in err, err
                assert raw_report(prover, K) == (0, want[0], chal or [0, 0, 0], want[1], want[2])
            prover.set_tuning("witness_kernel", 1)
            with pytest.raises(native.WitnessError) as e:
                prover.stark_prove(air.name, blob, d_bad, pubs, *ARGS)
            assert str(e.value) == err                     # WitnessReport's line is the library's, word for word
            assert e.value.report.counts == want[1] and e.value.report.first_constraint == want[0][2] and e.value.report.chal == (chal or [0, 0, 0])
            honest_again()                                  # the ctx stays usable: the same bytes
            prover.set_tuning("prove_check", 0)             # today's behaviour: a text comes back, one no verifier accepts
            rc, text, _ = raw_prove(prover, air, blob, d_bad, pubs)
            assert rc == 0 and text and text != plain
            prover.set_tuning("prove_check", 1)
        if name in ("perm", "chunk16"):
            assert WC.oracle_report(blob, bads[-1], pubs, LOGN, recorded_challenge(air, bads[-1], pubs, tables))[0][1] == N - 1
    finally:
        prover.set_tuning("prove_check", 0)
        prover.set_tuning("witness_kernel", 1)
        d.free()
        d_bad.free()


def test_noncanonical_word_in_the_proof(prover, hip):
    air, blob, trace, pubs = WC.honest_case("chunk16", LOGN)
    register(hip, air)
    K = int(blob[8])
    bad = np.array(trace, dtype=np.uint64)
    bad[4, 77] = P
    d, d_ok = prover.upload(bad), prover.upload(np.ascontiguousarray(trace))
    try:
        prover.set_tuning("prove_check", 0)
        plain = raw_prove(prover, air, blob, d_ok, pubs)[1]
        prover.set_tuning("prove_check", 1)
        (rc, text, err), stages = stages_of(prover, lambda: raw_prove(prover, air, blob, d, pubs))
        assert rc == -7 and text is None and "column 4 at row 77" in err
        assert "witness_canonical" in stages and not {"lde", GEN, INTERP} & set(stages), stages      # nothing after the point of refusal
        assert raw_report(prover, K) == (0, [WC.NONCANONICAL, NONE, NONE, 0, 0, 1, 4, 77], [0, 0, 0], [0] * K, [NONE] * K)
        assert raw_prove(prover, air, blob, d_ok, pubs)[1] == plain
    finally:
        prover.set_tuning("prove_check", 0)
        d.free()
        d_ok.free()


def test_checked_proof_in_bn128_mode(hip):
    air, blob, trace, pubs = WC.honest_case("chunk16", LOGN)
    p = native.Prover(0)
    try:
        p.install_poseidon_bn254(17)
        p.set_air_kernel_witness(blob, hip._airlib_witness(air))
        d = p.upload(np.ascontiguousarray(trace))
        rc, plain, err = raw_prove(p, air, blob, d, pubs, bn=True)
        assert rc == 0, err
        p.set_tuning("prove_check", 1)
        for knob, ran in ((1, GEN), (0, INTERP)):
            p.set_tuning("witness_kernel", knob)
            (rc, text, err), stages = stages_of(p, lambda: raw_prove(p, air, blob, d, pubs, bn=True))
            assert rc == 0 and text == plain and ran in stages, err
        p.h2d(d, np.ascontiguousarray(WC.flipped(trace, 9, 100)))
        assert raw_prove(p, air, blob, d, pubs, bn=True)[0] == -7
        d.free()
    finally:
        p.close()


def test_sharded_prover_does_not_read_the_knob(prover):
    from test_gpu_sharded_native import run_ranks
    air, blob, trace, pubs = WC.honest_case("chunk16", LOGN)
    wl = air.width // 2

    def ranks(knob):
        def fn(r, p, c):
            p.set_tuning("prove_check", knob)
            d_l = p.upload(np.ascontiguousarray(trace[r * wl:(r + 1) * wl]))
            return c.stark_prove_sharded(air.name, blob, d_l, pubs, *ARGS)
        return run_ranks(2, fn)
    off, on = ranks(0), ranks(1)
    assert on == off and on[0] == on[1]
    d = prover.upload(np.ascontiguousarray(trace))
    assert prover.stark_prove(air.name, blob, d, pubs, *ARGS) == on[0]
    d.free()


# ---------------------------------------------------------------------------------------------- engine and compiled host
def engine_cfg(**kw):
    from eigen_zeth_amd.service.engine import EngineConfig
    return EngineConfig(air="chunk16", logn=8, n_queries=6, fri_final_log=3, pow_bits=4, chunks_per_block=1, prover_streams=2, **kw)


def test_engine_checks_in_the_proof(monkeypatch, tables):
    from eigen_zeth_amd.service.engine import Engine, WitnessError
    from eigen_zeth_amd.service.server import default_backend_factory
    from eigen_zeth_amd.stark import air as AIR

    def run(**kw):
        eng = Engine(default_backend_factory(0), engine_cfg(**kw))
        ch = eng.gen_batch_chunks("b", [3, 4], 12345, "evm")
        out = eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
        return eng, ch, [o["proof"] for o in out]
    _, _, off = run()
    eng, ch, on = run(check_witness="prove")
    assert on == off and len(on) == 2
    assert not any("witness_check" in tm for tm in eng.stage_timings.values())      # no separate call: the proof checked itself
    plan = json.loads(ch["batch_data"])["chunks"][0]
    air = AIR.get_air("chunk16")
    real = Engine._chunk_witness
    col, row = 9, 100

    def corrupted(a, c, out=None):
        tr, pubs = real(a, c, out)
        tr[col, row] = (int(tr[col, row]) + 1) % P
        return tr, pubs
    tr, pubs = real(air, plan)
    bad, pl = WC.flipped(tr, col, row), [int(v) for v in pubs]
    chal = recorded_challenge(air, bad, pl, tables, eng.stark_params(plan["logn"]))
    want = WC.oracle_report(np.asarray(air.program(), dtype=np.uint64), bad, pl, plan["logn"], chal)
    assert want[0][0] == WC.VIOLATED
    monkeypatch.setattr(Engine, "_chunk_witness", staticmethod(corrupted))
    with pytest.raises(WitnessError) as e:
        eng.gen_chunk_proofs("c", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    assert "constraint %d at row %d" % (want[0][2], want[0][1]) in str(e.value) and e.value.report.counts == want[1]
    assert "c" not in eng._batch_chunk_proofs


def test_compiled_host_check_prove_flag(tmp_path, prover):
    """host/prove_chunk --check-prove: the report of the proof's own check as one JSON line in front of the result; a refusal ends the run with
    status 3, unproven"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "prove_chunk")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s"])
    logn = 8
    air, blob, trace, pubs = WC.honest_case("chunk16", logn)
    blob.tofile(tmp_path / "program.bin")
    np.asarray(pubs, dtype=np.uint64).tofile(tmp_path / "publics.bin")
    d = prover.upload(np.ascontiguousarray(trace))
    plain = prover.stark_prove(air.name, blob, d, pubs, logn, 1, 3, 3, 6, 4)
    d.free()

    def run(tr, name):
        np.ascontiguousarray(tr, dtype=np.uint64).tofile(tmp_path / "trace.bin")
        out = tmp_path / name
        r = subprocess.run([exe, "--check-prove", str(tmp_path / "program.bin"), str(tmp_path / "trace.bin"), str(tmp_path / "publics.bin"), str(logn), "1", "3", "3",
                            "6", "4", str(out), air.name], capture_output=True, text=True, timeout=120)
        return r, out, json.loads(r.stdout.splitlines()[0])["witness_check"]
    r, out, rep = run(trace, "good.json")
    assert r.returncode == 0, r.stdout + r.stderr
    assert rep == {"verdict": "satisfied", "first_row": None, "first_constraint": None, "violations": 0, "violated_constraints": 0, "noncanonical": 0,
                   "first_noncanonical": None}
    assert out.read_text() == plain
    bad = WC.flipped(trace, 1, 100)                        # a wide-mix column: no stage-2 constraint reads it, the verdict does not depend on the challenge
    want = WC.oracle_report(blob, bad, pubs, logn)
    r, out, rep = run(bad, "bad.json")
    assert r.returncode == 3 and not out.exists()
    assert (rep["verdict"], rep["first_row"], rep["first_constraint"], rep["violations"], rep["violated_constraints"]) == ("violated",) + tuple(want[0][1:5])
    bad = np.array(trace, dtype=np.uint64)
    bad[4, 77] = P
    r, out, rep = run(bad, "noncanonical.json")
    assert r.returncode == 3 and not out.exists() and rep["verdict"] == "noncanonical" and rep["noncanonical"] == 1 and rep["first_noncanonical"] == [4, 77]
