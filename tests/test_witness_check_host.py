"""zp_stark_check_witness without a ctx (csrc/witness_host.hip; no GPU): report, counts and first rows against the checker's own row walk
(tests/witness_cases.py: oracle/air_program.py's Program.evaluate_base with fixed_period, the two selectors and NV.root) -- exact integers, no
tolerance -- then the refusals and the engine's check_witness flag on the tests' CPU backend."""
import ctypes as C
import json

import numpy as np
import pytest

import program_cases as PC
import witness_cases as WC
from eigen_zeth_amd import native
from oracle.air_program import Program

P = WC.P
NONE = WC.NONE
_u64p = C.POINTER(C.c_uint64)


def raw_check(ctx, blob, trace_ptr, trace_words, pubs, logn, chal=None, n_constraints=None, threads=0, want_arrays=True, n_pubs=None):
    """the C call itself: (rc, report[8], counts[K], first_rows[K]) with the outputs pre-filled by a pattern (untouched outputs are visible)"""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    K = int(blob[8]) if blob.size > 8 and int(blob[8]) < (1 << 20) else 1
    pb = np.array([int(v) for v in pubs] + [0], dtype=np.uint64)
    ch = None if chal is None else np.array([int(v) for v in chal], dtype=np.uint64)
    rep, counts, first = (np.full(n, 0xA5A5A5A5, dtype=np.uint64) for n in (8, max(K, 1), max(K, 1)))
    p = lambda a: a.ctypes.data_as(_u64p)
    rc = native.load_library().zp_stark_check_witness(ctx, p(blob), blob.size, trace_ptr, trace_words, p(pb), len(pubs) if n_pubs is None else n_pubs, logn,
                                                      None if ch is None else p(ch), p(rep), p(counts) if want_arrays else None,
                                                      p(first) if want_arrays else None, K if n_constraints is None else n_constraints, threads)
    return rc, [int(v) for v in rep], [int(v) for v in counts[:K]], [int(v) for v in first[:K]]


def host_check(blob, trace, pubs, logn, chal=None, threads=0):
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    rc, rep, counts, first = raw_check(None, blob, tr.ctypes.data, tr.size, pubs, logn, chal, threads=threads)
    assert rc == 0
    return rep, counts, first


def test_vector_walk_is_the_row_walk():
    """the expectation's one call of evaluate_base over all rows equals evaluate_base called row by row"""
    for name in ("cover", "periods"):
        blob, trace, pubs, _ = WC.random_case(name, 4)
        prog, N = Program(blob), 16
        outs = WC.oracle_outs(blob, trace, pubs, 4)
        tr, fixed, pubchal, xml = WC.row_operands(prog, trace, pubs, 4)
        for r in range(N):
            row = prog.evaluate_base([c[r] for c in tr], [c[(r + 1) % N] for c in tr], [f[r] for f in fixed], pubchal, xml[r])
            assert [int(o[r]) for o in outs] == [int(v) for v in row]


@pytest.mark.parametrize("logn", [1, 4, 7])
@pytest.mark.parametrize("name", [c[0] for c in PC.CASES])
def test_random_programs(name, logn):
    """every seeded program on a random canonical trace: nearly every row violates (the all-fail side)"""
    blob, trace, pubs, want = WC.random_case(name, logn)
    assert want[0][0] == WC.VIOLATED and want[0][3] > (1 << logn) // 2
    assert host_check(blob, trace, pubs, logn) == want
    assert host_check(blob, trace, pubs, logn, threads=3) == want
    r = native.check_witness_host(blob, trace, pubs, logn)
    assert (r.verdict, r.first_row, r.first_constraint, r.violations, r.violated_constraints) == tuple(want[0][:5]) and not r.ok
    assert r.counts == want[1] and r.noncanonical == 0 and r.first_noncanonical is None
    assert "constraint %d at row %d" % (want[0][2], want[0][1]) in str(r) and "\n" not in str(r)


@pytest.mark.parametrize("logn", [4, 5, 6])
@pytest.mark.parametrize("name", WC.SATISFIED_AIRS)
def test_satisfied(name, logn):
    air, blob, trace, pubs = WC.honest_case(name, logn)
    K = int(blob[8])
    for chal in ([None, WC.EXPLICIT_CHALLENGE] if air.stage2 else [None]):
        want = WC.oracle_report(blob, trace, pubs, logn, chal)
        assert want == ([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K)
        assert host_check(blob, trace, pubs, logn, chal) == want
    assert native.check_witness_host(blob, trace, pubs, logn).ok


def flips(air, logn):
    """(column, row) of the flipped cells: row 0, row N - 1, a cell of the last column, one in the middle, the last row of the second column"""
    N = 1 << logn
    return [(0, 0), (0, N - 1), (air.width - 1, N - 1), (air.width // 2, N // 2 + 1), (1 % air.width, N - 1)]


@pytest.mark.parametrize("name", WC.SATISFIED_AIRS)
def test_one_word_flipped(name):
    logn = 5
    air, blob, trace, pubs = WC.honest_case(name, logn)
    for col, row in flips(air, logn):
        bad = WC.flipped(trace, col, row)
        want = WC.oracle_report(blob, bad, pubs, logn)
        assert want[0][0] == WC.VIOLATED, (col, row)
        assert host_check(blob, bad, pubs, logn) == want, (col, row)


def test_flip_semantics_on_fib():
    """fib: a' = b (0), b' = a + b (1), both times (x - last); a[0] = pub0 (2), b[0] = pub1 (3), b[N-1] = pub2 (4)"""
    logn, N = 5, 32
    _, blob, trace, pubs = WC.honest_case("fib", logn)
    # a[0]: its own first-row constraint and the transition that reads it at row 0 -- NOT transition 0 at row N - 1, which reads it through the
    # next-row operand: the factor is 0 there
    bad = WC.flipped(trace, 0, 0)
    assert WC.violated_pairs(blob, bad, pubs, logn) == {(2, 0), (1, 0)}
    rep, counts, first = host_check(blob, bad, pubs, logn)
    assert rep[:5] == [WC.VIOLATED, 0, 1, 2, 2] and counts == [0, 1, 1, 0, 0] and first == [NONE, 0, 0, NONE, NONE]
    # a[N-1]: read at its own row only under the zero factor; what fails is row N - 2, which reads it through the next-row operand
    bad = WC.flipped(trace, 0, N - 1)
    assert WC.violated_pairs(blob, bad, pubs, logn) == {(0, N - 2)}
    rep, counts, first = host_check(blob, bad, pubs, logn)
    assert rep[:5] == [WC.VIOLATED, N - 2, 0, 1, 1] and counts == [1, 0, 0, 0, 0] and first == [N - 2, NONE, NONE, NONE, NONE]
    # b[N-1]: the last-row constraint at row N - 1 and the transition at N - 2
    bad = WC.flipped(trace, 1, N - 1)
    assert WC.violated_pairs(blob, bad, pubs, logn) == {(1, N - 2), (4, N - 1)}
    assert host_check(blob, bad, pubs, logn) == WC.oracle_report(blob, bad, pubs, logn)


@pytest.mark.parametrize("logn", [4, 6])
def test_broken_stage2_arguments(logn):
    N = 1 << logn
    for make, wrap in ((WC.broken_perm, {1, 2, 3}), (WC.broken_lookup, None)):
        blob, bad, pubs = make(logn)
        for chal in (None, WC.EXPLICIT_CHALLENGE):
            want = WC.oracle_report(blob, bad, pubs, logn, chal)
            pairs = WC.violated_pairs(blob, bad, pubs, logn, chal)
            assert want[0][0] == WC.VIOLATED and want[0][1] == N - 1 and {r for _, r in pairs} == {N - 1}
            if wrap is not None:
                assert {k for k, _ in pairs} <= wrap            # only the wrap-around constraints Z' (b + g) = Z (a + g)
            assert host_check(blob, bad, pubs, logn, chal) == want


def test_noncanonical_words():
    logn, N = 5, 32
    air, blob, trace, pubs = WC.honest_case("wide8", logn)
    K = int(blob[8])
    for cells, first in (([(0, 3, P), (7, N - 1, (1 << 64) - 1)], (0, 3)), ([(5, 0, (1 << 64) - 1), (2, 9, P)], (2, 9)),
                         ([(7, N - 1, P)], (7, N - 1)), ([(0, 0, P), (0, 1, P + 1), (3, 3, P)], (0, 0))):
        bad = np.array(trace, dtype=np.uint64)
        for c, r, v in cells:
            bad[c, r] = v
        want = ([WC.NONCANONICAL, NONE, NONE, 0, 0, len(cells), first[0], first[1]], [0] * K, [NONE] * K)
        assert WC.oracle_report(blob, bad, pubs, logn) == want
        assert host_check(blob, bad, pubs, logn) == want
        r = native.check_witness_host(blob, bad, pubs, logn)
        assert r.verdict == native.WITNESS_NONCANONICAL and r.noncanonical == len(cells) and r.first_noncanonical == first
        assert "column %d at row %d" % first in str(r)
    # p - 1 is canonical
    ok = WC.flipped(trace, 0, 0, 0)
    ok[7, 5] = P - 1
    assert host_check(blob, ok, pubs, logn)[0][0] == WC.VIOLATED


def refusal_base():
    """the good blob tests/test_program_cases.py cuts its malformed ones from, with a trace on 2^5 rows"""
    blob, shape = PC.gen(110, 5, width=3, n_pub=4, n_const=5, n_slots=6, K=4, n_body=20, lps=(2, 1), fills=("full", "pub"))
    trace, pubs = WC.random_inputs(shape, 5, 4242)
    return blob, shape, trace, pubs


UNTOUCHED = ([0xA5A5A5A5] * 8,)


def refused(blob, trace, words, pubs, logn, **kw):
    rc, rep, counts, first = raw_check(None, blob, trace.ctypes.data, words, pubs, logn, **kw)
    assert rc == -1
    assert rep == [0xA5A5A5A5] * 8 and set(counts) | set(first) == {0xA5A5A5A5}


def test_refusals():
    blob, shape, trace, pubs = refusal_base()
    rc, rep, _, _ = raw_check(None, blob, trace.ctypes.data, trace.size, pubs, 5)
    assert rc == 0 and rep[0] == WC.VIOLATED
    classes = list(PC.malformed(blob, shape))
    const_p = blob.copy()
    const_p[12 + 2] = P
    classes.append(("constant_value_p", const_p))
    slots33 = blob.copy()
    slots33[9] = 33
    classes.append(("slots_33", slots33))
    assert len(classes) == 22
    for cls, bad in classes:
        refused(bad, trace, trace.size, pubs, 5)
    # the arguments
    refused(blob, trace, trace.size - 1, pubs, 5)                       # trace_words != W * 2^logn
    refused(blob, trace, trace.size, pubs, 4)
    refused(blob, trace, trace.size, pubs, 6)
    refused(blob, trace, trace.size, pubs[:-1], 5)                      # n_pubs not the program's
    refused(blob, trace, trace.size, pubs + [1], 5)
    refused(blob, trace, trace.size, pubs, 5, n_pubs=-1)
    refused(blob, trace, trace.size, [P] + pubs[1:], 5)                 # public input >= p
    refused(blob, trace, trace.size, pubs[:-1] + [(1 << 64) - 1], 5)
    refused(blob, trace, trace.size, pubs, 5, n_constraints=3)          # arrays given, n_constraints != K
    refused(blob, trace, trace.size, pubs, 5, n_constraints=5)
    refused(blob, trace, 3, pubs, 0)                                    # logn < 1
    refused(blob, trace, 0, pubs, -1)
    blob1, shape1 = PC.gen(110, 5, width=3, n_pub=4, n_const=5, n_slots=6, K=4, n_body=20, lps=(2, 1), fills=("full", "pub"))
    refused(blob1, trace, 3 << 1, pubs, 1)                              # a sparse column with lp = 2 > logn = 1
    # without the arrays n_constraints is not looked at
    rc, rep, _, _ = raw_check(None, blob, trace.ctypes.data, trace.size, pubs, 5, n_constraints=99, want_arrays=False)
    assert rc == 0 and rep[0] == WC.VIOLATED
    # a challenge word >= p (stage-2 program)
    _, pblob, ptrace, ppubs = WC.honest_case("perm", 4)
    pt = np.ascontiguousarray(ptrace)
    for chal in ([P, 0, 0], [0, (1 << 64) - 1, 0], [1, 2, P]):
        refused(pblob, pt, pt.size, ppubs, 4, chal=chal)
    with pytest.raises(native.ZpError):
        native.check_witness_host(blob, trace, pubs[:-1], 5)


# ---- the engine: EngineConfig(check_witness=True) on the tests' CPU backend
@pytest.fixture()
def cpu_factory(tables):
    from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
    from cpu_wrap_backend import CpuWrapBackend
    return lambda hash_mode="gl": CpuWrapBackend(*tables, hash_mode=hash_mode, bn_tables=bn254_poseidon_params(17) if hash_mode == "bn128" else None)


def engine_cfg(**kw):
    from eigen_zeth_amd.service.engine import EngineConfig
    return EngineConfig(air="chunk16", logn=5, n_queries=2, fri_final_log=3, pow_bits=4, chunks_per_block=1, prover_streams=2, **kw)


def test_engine_good_batch_is_byte_identical(cpu_factory):
    from eigen_zeth_amd.service.engine import Engine

    def run(**kw):
        eng = Engine(cpu_factory, engine_cfg(**kw))
        ch = eng.gen_batch_chunks("b", [3, 4], 12345, "evm")
        out = eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
        return [o["proof"] for o in out], eng.stage_timings
    off, tm_off = run()
    on, tm_on = run(check_witness=True)
    assert on == off and len(on) == 2
    assert all("witness_check" in tm for tm in tm_on.values()) and not any("witness_check" in tm for tm in tm_off.values())


def test_engine_refuses_a_corrupted_witness(cpu_factory, monkeypatch):
    from eigen_zeth_amd.service.engine import Engine, WitnessError
    from eigen_zeth_amd.stark import air as AIR
    eng = Engine(cpu_factory, engine_cfg(check_witness=True))
    ch = eng.gen_batch_chunks("b", [3], 12345, "evm")
    plan = json.loads(ch["batch_data"])["chunks"][0]
    air = AIR.get_air("chunk16")
    real = Engine._chunk_witness
    col, row = 2, 9

    def corrupted(a, c, out=None):
        tr, pubs = real(a, c, out)
        tr[col, row] = (int(tr[col, row]) + 1) % P
        return tr, pubs
    tr, pubs = real(air, plan)
    bad = WC.flipped(tr, col, row)
    want = WC.oracle_report(np.asarray(air.program(), dtype=np.uint64), bad, [int(v) for v in pubs], plan["logn"])
    assert want[0][0] == WC.VIOLATED
    monkeypatch.setattr(Engine, "_chunk_witness", staticmethod(corrupted))
    with pytest.raises(WitnessError) as e:
        eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    assert "constraint %d at row %d" % (want[0][2], want[0][1]) in str(e.value)
    assert (e.value.report.first_constraint, e.value.report.first_row, e.value.report.counts) == (want[0][2], want[0][1], want[1])
    assert "b" not in eng._batch_chunk_proofs
    # with the flag off the same witness is proven as before: a text comes back (one no verifier accepts)
    eng_off = Engine(cpu_factory, engine_cfg())
    assert len(eng_off.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])) == 1


def test_service_answers_a_corrupted_witness_by_its_error_convention(tmp_path, cpu_factory, monkeypatch):
    """GenChunkProof over a witness that violates its AIR: COMPLETED_ERROR, the report's line as the message, no result"""
    from eigen_zeth_amd.service import proto
    from eigen_zeth_amd.service.engine import Engine
    from eigen_zeth_amd.service.server import ProverService
    from eigen_zeth_amd.service.store import BatchStore
    eng = Engine(cpu_factory, engine_cfg(check_witness=True))
    svc = ProverService(eng, BatchStore(str(tmp_path)))
    ch = eng.gen_batch_chunks("b", [3], 12345, "evm")
    real = Engine._chunk_witness

    def corrupted(a, c, out=None):
        tr, pubs = real(a, c, out)
        tr[2, 9] = (int(tr[2, 9]) + 1) % P
        return tr, pubs
    monkeypatch.setattr(Engine, "_chunk_witness", staticmethod(corrupted))
    req = proto.ProverRequest(id="x")
    g = req.gen_batch_proof.gen_chunk_proof
    g.batch_id, g.task_id, g.chunk_count, g.batch_data = "b", ch["task_id"], ch["chunk_count"], ch["batch_data"]
    resp, = list(svc.prover_stream(iter([req]), None))
    r = resp.gen_batch_proof.gen_chunk_proof
    assert r.result_code == proto.COMPLETED_ERROR and not r.HasField("batch_proof_result")
    assert r.error_message.startswith("WitnessError: witness violates constraint ") and " at row " in r.error_message


def test_recursion_statement():
    """the statement of the recursion STARKs (what check_witness=True judges in front of the aggregation and the final STARK): a verifier AIR with
    its ~100 sparse fixed columns and public-input entries, its own witness and one cell of it flipped"""
    blob, trace, pubs, logn = WC.verifier_air_case()
    assert int(blob[3]) > 50 and int(blob[9]) <= 32
    K = int(blob[8])
    assert host_check(blob, trace, pubs, logn) == ([WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE], [0] * K, [NONE] * K)
    bad = WC.flipped(trace, 30, 77)
    want = WC.oracle_report(blob, bad, pubs, logn)
    assert want[0][0] == WC.VIOLATED
    assert host_check(blob, bad, pubs, logn) == want
