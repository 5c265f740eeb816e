"""zp_stark_check_witness on a ctx (csrc/witness_check.hip: witness_canonical_kernel, witness_program_kernel, the stage-2 columns by the prover's
primitives): report, counts and first rows equal the host path's (ctx = NULL) and the checker's own row walk (tests/witness_cases.py) word for
word -- exact integers -- at every size at which the kernel takes another shape: N = 2 (logn 1), less than a wave (5), one wave (6), one workgroup
(8), two (9), sixteen (12)."""
import json

import numpy as np
import pytest

import program_cases as PC
import witness_cases as WC
from test_witness_check_host import host_check, raw_check
from eigen_zeth_amd import native

pytestmark = pytest.mark.gpu

P = WC.P
NONE = WC.NONE


def device_check(prover, blob, trace, pubs, logn, chal=None):
    """(report, counts, first rows) through the ctx; the trace must come back unchanged"""
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    d = prover.upload(tr)
    try:
        rc, rep, counts, first = raw_check(prover.ctx, blob, d.ptr, tr.size, pubs, logn, chal)
        assert rc == 0, prover.lib.zp_last_error(prover.ctx)
        assert (prover.download(d, tr.shape) == tr).all()
    finally:
        d.free()
    return rep, counts, first


def agree(prover, blob, trace, pubs, logn, chal=None, want=None):
    want = WC.oracle_report(blob, trace, pubs, logn, chal) if want is None else want
    assert host_check(blob, trace, pubs, logn, chal) == want
    assert device_check(prover, blob, trace, pubs, logn, chal) == want
    return want


@pytest.mark.parametrize("logn", [1, 5, 6, 8, 9])
def test_random_programs(prover, logn):
    for name in [c[0] for c in PC.CASES]:
        blob, trace, pubs, want = WC.random_case(name, logn)
        assert want[0][0] == WC.VIOLATED
        agree(prover, blob, trace, pubs, logn, want=want)


@pytest.mark.parametrize("logn", [6, 9])
def test_satisfied_flipped_and_stage2(prover, logn):
    N = 1 << logn
    for name in WC.SATISFIED_AIRS:
        air, blob, trace, pubs = WC.honest_case(name, logn)
        for chal in ([None, WC.EXPLICIT_CHALLENGE] if air.stage2 else [None]):
            assert agree(prover, blob, trace, pubs, logn, chal)[0][0] == WC.SATISFIED
        for col, row in [(0, 0), (0, N - 1), (air.width - 1, N - 1), (air.width // 2, N // 2 + 1)]:
            assert agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)[0][0] == WC.VIOLATED
    for make in (WC.broken_perm, WC.broken_lookup):
        blob, bad, pubs = make(logn)
        for chal in (None, WC.EXPLICIT_CHALLENGE):
            want = agree(prover, blob, bad, pubs, logn, chal)
            assert want[0][0] == WC.VIOLATED and want[0][1] == N - 1


def test_flips_at_wave_and_workgroup_seams(prover):
    logn = 9
    for name in ("fib", "chunk16"):
        air, blob, trace, pubs = WC.honest_case(name, logn)
        for row in (63, 64, 255, 256):
            for col in (0, air.width - 1):
                want = agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)
                assert want[0][0] == WC.VIOLATED and row - 1 <= want[0][1] <= row
    # fib: a[row] is read through the next-row operand by row - 1 (a' = b) and at its own row by b' = a + b
    _, blob, trace, pubs = WC.honest_case("fib", logn)
    for row in (64, 256):
        rep, counts, first = device_check(prover, blob, WC.flipped(trace, 0, row), pubs, logn)
        assert rep[:5] == [WC.VIOLATED, row - 1, 0, 2, 2] and counts == [1, 1, 0, 0, 0] and first == [row - 1, row, NONE, NONE, NONE]


def test_all_rows_violate_at_logn_12(prover):
    """counts must equal N exactly: the ballot aggregation over 64 waves and the dead-lane mask"""
    logn, N = 12, 1 << 12
    blob, trace, pubs, want = WC.random_case("one_slot_one_constraint", logn)
    assert want == ([WC.VIOLATED, 0, 0, N, 1, 0, NONE, NONE], [N], [0])
    agree(prover, blob, trace, pubs, logn, want=want)
    for name in ("bounded_c", "no_publics"):
        blob, trace, pubs, want = WC.random_case(name, logn)
        assert all(c == N for c in want[1])
        agree(prover, blob, trace, pubs, logn, want=want)
    # ... and below a workgroup: N = 32 live lanes of 256
    blob, trace, pubs, want = WC.random_case("one_slot_one_constraint", 5)
    assert want[1] == [32]
    assert device_check(prover, blob, trace, pubs, 5) == want


def test_chunk64_at_logn_12(prover):
    logn = 12
    air, blob, trace, pubs = WC.honest_case("chunk64", logn)
    K = int(blob[8])
    want = agree(prover, blob, trace, pubs, logn)          # the derived challenge
    assert want == ([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K)
    bad = WC.flipped(trace, 17, 1000)                       # a wide-mix column
    want = agree(prover, blob, bad, pubs, logn)
    assert want[0][0] == WC.VIOLATED and want[0][1] == 999 and WC.violated_pairs(blob, bad, pubs, logn) == {(17, 999), (15, 1000), (16, 1000), (17, 1000)}


def test_noncanonical_words(prover):
    logn, N = 9, 512
    air, blob, trace, pubs = WC.honest_case("wide8", logn)
    K = int(blob[8])
    # the blob's instructions never name a column >= 8: a statement over the first 8 columns of a 9-column trace leaves column 8 unread
    for cells, first in (([(0, 0, P)], (0, 0)), ([(7, N - 1, (1 << 64) - 1)], (7, N - 1)), ([(0, 0, P), (7, N - 1, P)], (0, 0)),
                         ([(3, 300, P + 5), (2, 511, (1 << 64) - 1), (6, 1, P)], (2, 511))):
        bad = np.array(trace, dtype=np.uint64)
        for c, r, v in cells:
            bad[c, r] = v
        want = ([WC.NONCANONICAL, NONE, NONE, 0, 0, len(cells), first[0], first[1]], [0] * K, [NONE] * K)
        agree(prover, blob, bad, pubs, logn, want=want)
    # a column no instruction reads: the program of "one_slot_one_constraint" widened by a column nothing names
    blob1, trace1, pubs1, _ = WC.random_case("one_slot_one_constraint", 6)
    wide = blob1.copy()
    wide[1] = 2
    tr2 = np.concatenate([trace1, trace1]).reshape(2, 64)
    assert agree(prover, wide, tr2, pubs1, 6)[0][0] == WC.VIOLATED
    tr2[1, 40] = P
    agree(prover, wide, tr2, pubs1, 6, want=([WC.NONCANONICAL, NONE, NONE, 0, 0, 1, 1, 40], [0], [NONE]))
    # an odd word offset into the buffer (8-byte aligned only): the pass takes its first word alone
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    bad = tr.copy()
    bad[0, 0], bad[7, N - 1] = P, P
    d = prover.alloc(tr.size + 1)
    try:
        prover.h2d(d.offset(1), bad)
        rc, rep, _, _ = raw_check(prover.ctx, blob, d.offset(1), tr.size, pubs, logn)
        assert rc == 0 and rep == [WC.NONCANONICAL, NONE, NONE, 0, 0, 2, 0, 0]
        prover.h2d(d.offset(1), tr)
        rc, rep, _, _ = raw_check(prover.ctx, blob, d.offset(1), tr.size, pubs, logn)
        assert rc == 0 and rep[0] == WC.SATISFIED
    finally:
        d.free()


def test_refusals_on_a_ctx(prover):
    from test_witness_check_host import refusal_base
    blob, shape, trace, pubs = refusal_base()
    d = prover.upload(trace)
    try:
        for cls, bad in PC.malformed(blob, shape):
            rc, rep, counts, first = raw_check(prover.ctx, bad, d.ptr, trace.size, pubs, 5)
            assert rc == -1 and rep == [0xA5A5A5A5] * 8 and set(counts) | set(first) == {0xA5A5A5A5}, cls
        for kw in (dict(words=trace.size - 1), dict(logn=4), dict(pubs=pubs[:-1]), dict(pubs=[P] + pubs[1:]), dict(n_constraints=3)):
            rc, rep, _, _ = raw_check(prover.ctx, blob, d.ptr, kw.get("words", trace.size), kw.get("pubs", pubs), kw.get("logn", 5),
                                      n_constraints=kw.get("n_constraints"))
            assert rc == -1 and rep == [0xA5A5A5A5] * 8, kw
        with pytest.raises(native.ZpError):
            prover.check_witness(blob, d, pubs[:-1], 5)
        assert prover.check_witness(blob, d, pubs, 5).verdict == native.WITNESS_VIOLATED       # the ctx still works
    finally:
        d.free()


def test_check_then_prove_on_the_same_buffer(prover):
    """Prover.check_witness followed by stark_prove on the same device buffer: the proof of a prover that never checked"""
    from eigen_zeth_amd.stark import prover as PR
    logn = 8
    air, blob, trace, pubs = WC.honest_case("chunk16", logn)
    params = PR.StarkParams(logn, 1, 3, 3, 6, pow_bits=4)
    args = (params.logn, params.logb, params.fri_logf, params.fri_final_log, params.n_queries, params.pow_bits)
    d = prover.upload(np.ascontiguousarray(trace))
    plain = prover.stark_prove(air.name, blob, d, pubs, *args)
    d.free()
    d = prover.upload(np.ascontiguousarray(trace))
    rep = prover.check_witness(blob, d, pubs, logn)
    assert rep.ok and rep.counts == [0] * int(blob[8]) and str(rep).startswith("witness satisfies")
    checked = prover.stark_prove(air.name, blob, d, pubs, *args)
    assert (prover.download(d, trace.shape) == trace).all()
    d.free()
    assert checked == plain


def engine_cfg(**kw):
    from eigen_zeth_amd.service.engine import EngineConfig
    return EngineConfig(air="chunk16", logn=8, n_queries=6, fri_final_log=3, pow_bits=4, chunks_per_block=1, prover_streams=2, **kw)


def test_engine_on_the_hip_backend(monkeypatch):
    from eigen_zeth_amd.service.engine import Engine, WitnessError
    from eigen_zeth_amd.service.server import default_backend_factory
    from eigen_zeth_amd.stark import air as AIR

    def run(**kw):
        eng = Engine(default_backend_factory(0), engine_cfg(**kw))
        ch = eng.gen_batch_chunks("b", [3, 4], 12345, "evm")
        out = eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
        return eng, ch, [o["proof"] for o in out]
    _, _, off = run()
    eng, ch, on = run(check_witness=True)
    assert on == off and len(on) == 2
    assert all("witness_check" in tm for tm in eng.stage_timings.values())
    plan = json.loads(ch["batch_data"])["chunks"][0]
    air = AIR.get_air("chunk16")
    real = Engine._chunk_witness
    col, row = 9, 100

    def corrupted(a, c, out=None):
        tr, pubs = real(a, c, out)
        tr[col, row] = (int(tr[col, row]) + 1) % P
        return tr, pubs
    tr, pubs = real(air, plan)
    want = WC.oracle_report(np.asarray(air.program(), dtype=np.uint64), WC.flipped(tr, col, row), [int(v) for v in pubs], plan["logn"])
    assert want[0][0] == WC.VIOLATED
    monkeypatch.setattr(Engine, "_chunk_witness", staticmethod(corrupted))
    with pytest.raises(WitnessError) as e:
        eng.gen_chunk_proofs("c", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    assert "constraint %d at row %d" % (want[0][2], want[0][1]) in str(e.value) and e.value.report.counts == want[1]
    assert "c" not in eng._batch_chunk_proofs


def test_compiled_host_check_flag(tmp_path, prover):
    """host/prove_chunk --check: the report as one JSON line in front of the proof; a violated or non-canonical trace ends the run with status 3, unproven"""
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
        r = subprocess.run([exe, "--check", str(tmp_path / "program.bin"), str(tmp_path / "trace.bin"), str(tmp_path / "publics.bin"), str(logn), "1", "3", "3", "6", "4",
                            str(out), air.name], capture_output=True, text=True, timeout=120)
        return r, out, json.loads(r.stdout.splitlines()[0])["witness_check"]
    r, out, rep = run(trace, "good.json")
    assert r.returncode == 0, r.stdout + r.stderr
    assert rep == {"verdict": "satisfied", "first_row": None, "first_constraint": None, "violations": 0, "violated_constraints": 0, "noncanonical": 0,
                   "first_noncanonical": None}
    assert out.read_text() == plain
    bad = WC.flipped(trace, 9, 100)
    want = WC.oracle_report(blob, bad, pubs, logn)
    r, out, rep = run(bad, "bad.json")
    assert r.returncode == 3 and not out.exists()
    assert (rep["verdict"], rep["first_row"], rep["first_constraint"], rep["violations"], rep["violated_constraints"]) == ("violated",) + tuple(want[0][1:5])
    bad = np.array(trace, dtype=np.uint64)
    bad[4, 77] = P
    r, out, rep = run(bad, "noncanonical.json")
    assert r.returncode == 3 and not out.exists() and rep["verdict"] == "noncanonical" and rep["noncanonical"] == 1 and rep["first_noncanonical"] == [4, 77]


def test_recursion_statement(prover):
    """a verifier AIR (the statement of the aggregation and the final STARK): ~100 sparse fixed columns read through the (offset, mask) table"""
    blob, trace, pubs, logn = WC.verifier_air_case()
    K = int(blob[8])
    agree(prover, blob, trace, pubs, logn, want=([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K))
    for col, row in ((30, 77), (0, 0), (46, (1 << logn) - 1), (12, 2048)):
        assert agree(prover, blob, WC.flipped(trace, col, row), pubs, logn)[0][0] == WC.VIOLATED
