"""zp_stark_diagnose_stage2 without a ctx (csrc/stage2_diag_host.hip; no GPU): every record against the multiset comparison of
tests/stage2_diag_cases.py, word for word -- exact integers -- then the refusals, the agreement with zp_stark_check_witness on which traces
fail, and the engine's diagnose_stage2 flag on the tests' CPU backend."""
import ctypes as C
import json

import numpy as np
import pytest

import program_cases as PC
import stage2_diag_cases as SC
import witness_cases as WC
from eigen_zeth_amd import native

P = WC.P
NONE = WC.NONE
MARK = 0xA5A5A5A5
_u64p = C.POINTER(C.c_uint64)


def raw_diag(ctx, blob, trace_ptr, trace_words, logn, n_stage2=None, threads=0):
    """the C call itself: (rc, [record of 12 ints] per argument of the blob's header) with the output pre-filled by a pattern"""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    n = int(blob[10]) if blob.size > 10 and int(blob[10]) < (1 << 12) else 0
    out = np.full(max(n, 1) * SC.WORDS, MARK, dtype=np.uint64)
    rc = native.load_library().zp_stark_diagnose_stage2(ctx, blob.ctypes.data_as(_u64p), blob.size, trace_ptr, trace_words, logn, out.ctypes.data_as(_u64p),
                                                        n if n_stage2 is None else n_stage2, threads)
    return rc, [[int(v) for v in out[SC.WORDS * j:SC.WORDS * (j + 1)]] for j in range(max(n, 1))]


def host_diag(blob, trace, logn, threads=0):
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    keep = tr.copy()
    rc, recs = raw_diag(None, blob, tr.ctypes.data, tr.size, logn, threads=threads)
    assert rc == 0 and (tr == keep).all()
    return recs


@pytest.mark.parametrize("name,logn", SC.all_cases())
def test_records_equal_the_expectation(name, logn):
    blob, trace, _ = SC.case(name, logn)
    want = SC.expected(blob, trace, logn)
    assert host_diag(blob, trace, logn, threads=1) == want
    if logn >= 12:        # the values shared out over threads: the same words
        assert host_diag(blob, trace, logn, threads=3) == want and host_diag(blob, trace, logn) == want


def check_semantics(diag, logn):
    """the properties the case set was built for, on whatever `diag(blob, trace, logn)` computes them"""
    N = 1 << logn
    for name in ("honest_perm", "honest_chunk16"):
        blob, trace, _ = SC.case(name, logn)
        for rec in diag(blob, trace, logn):
            assert rec[0] == SC.HOLDS and rec[2] == rec[11] == 0 and rec[3] == rec[7] == NONE
    blob, trace, row = SC.case("broken_perm", logn)
    (rec,) = diag(blob, trace, logn)
    assert rec[:3] == [SC.FAILS, 1, 2] and rec[7] == row and rec[8] == int(trace[1, row]) and rec[9:11] == [0, 1]
    blob, trace, row = SC.case("broken_lookup", logn)
    perm, look = diag(blob, trace, logn)
    assert perm[0] == SC.HOLDS and look[:2] == [SC.FAILS, 2]
    # r_a is the edited row, its value in a once and in the table never -- unless the value that was taken out (now hit once less than its
    # multiplicity says, so unbalanced too) also stands in an earlier row of a
    a = SC.arguments(blob)[1]["a"]
    old = SC.case("honest_chunk16", logn)[1][a, row]
    earlier = [int(r) for r in np.nonzero(trace[a, :row] == old)[0]]
    if earlier:
        assert look[2] == 2 and look[3:5] == [earlier[0], int(old)] and look[6] == look[5] + 1
    else:
        assert look[3] == row and look[4] == int(trace[a, row]) and look[5:7] == [1, 0]
    blob, trace, _ = SC.case("disjoint", logn)
    (rec,) = diag(blob, trace, logn)
    assert rec == [SC.FAILS, 1, 2 * N, 0, 0, 1, 0, 0, N, 0, 1, N]
    blob, trace, _ = SC.case("noncanonical", logn)
    assert diag(blob, trace, logn) == [[SC.NONCANONICAL, k, 0, NONE, NONE, 0, 0, NONE, NONE, 0, 0, 0] for k in (1, 2)]
    if logn < 5:
        return
    blob, trace, i = SC.case("multiplicity", logn)
    look = SC.arguments(blob)[1]
    perm_rec, rec = diag(blob, trace, logn)
    assert perm_rec[0] == SC.HOLDS and rec[:3] == [SC.FAILS, 2, 2]
    assert rec[7] == i and rec[8] == int(trace[look["b"], i]) and rec[10] == rec[9] + 1
    first = lambda v: int(np.nonzero(trace[look["a"]] == v)[0][0])
    k = [int(x) for x in np.nonzero(SC.case("honest_chunk16", logn)[1][look["m"]] != 0)[0]][-1]       # the row whose m went down
    assert rec[3] == min(first(trace[look["b"], i]), first(trace[look["b"], k]))
    c = N // 2
    blob, trace, _ = SC.case("m_mod_p", logn)
    assert [r[0] for r in diag(blob, trace, logn)] == [SC.HOLDS, SC.HOLDS]
    blob, trace, _ = SC.case("m_mod_p_off", logn)
    assert diag(blob, trace, logn)[1] == [SC.FAILS, 2, 1, 0, 7, c, c - 1, 0, 7, c, c - 1, c]
    blob, trace, _ = SC.case("one_value", logn)
    assert [r[0] for r in diag(blob, trace, logn)] == [SC.HOLDS, SC.HOLDS]
    blob, trace, _ = SC.case("one_value_short", logn)
    assert diag(blob, trace, logn)[1] == [SC.FAILS, 2, 1, 0, 5, N, N - 1, 0, 5, N, N - 1, N]
    for kind in SC.COLLISIONS:
        blob, trace, _ = SC.case("collide:%s:whole" % kind, logn)
        assert diag(blob, trace, logn)[0][:3] == [SC.HOLDS, 1, 0]
        blob, trace, _ = SC.case("collide:%s:broken" % kind, logn)
        assert diag(blob, trace, logn)[0][:3] == [SC.FAILS, 1, 2]


@pytest.mark.parametrize("logn", SC.LOGNS)
def test_what_the_cases_mean(logn):
    check_semantics(lambda blob, trace, lg: host_diag(blob, trace, lg), logn)
    check_semantics(SC.expected, logn)


def check_refusals(ctx, ptr_of):
    """every refusal of include/zeth_prover.h returns ZP_ERR_ARG and leaves the output as it was; ptr_of(array) -> (pointer, release)"""
    def refused(blob, ptr, words, logn, **kw):
        rc, recs = raw_diag(ctx, blob, ptr, words, logn, **kw)
        assert rc == -1 and all(set(r) == {MARK} for r in recs), (rc, kw)
    # a program without arguments: its malformed forms, and n_stage2 = 0 on the good one
    blob, shape = PC.gen(110, 5, width=3, n_pub=4, n_const=5, n_slots=6, K=4, n_body=20, lps=(2, 1), fills=("full", "pub"))
    trace, _ = WC.random_inputs(shape, 5, 4242)
    ptr, release = ptr_of(trace)
    try:
        classes = list(PC.malformed(blob, shape))
        assert len(classes) == 20
        for _, bad in classes:
            refused(bad, ptr, trace.size, 5)
        refused(blob, ptr, trace.size, 5, n_stage2=1)
        rc, recs = raw_diag(ctx, blob, ptr, trace.size, 5)
        assert rc == 0 and set(recs[0]) == {MARK}                  # ZP_OK, nothing written
    finally:
        release()
    _, fib, ftrace, _ = WC.honest_case("fib", 5)
    ptr, release = ptr_of(ftrace)
    try:
        rc, recs = raw_diag(ctx, fib, ptr, ftrace.size, 5)
        assert rc == 0 and set(recs[0]) == {MARK}
    finally:
        release()
    # a program with two
    _, blob, trace, _ = WC.honest_case("chunk16", 5)
    ptr, release = ptr_of(trace)
    try:
        assert raw_diag(ctx, blob, ptr, trace.size, 5)[0] == 0
        refused(blob, ptr, trace.size - 1, 5)                      # trace_words != W * 2^logn
        refused(blob, ptr, trace.size, 4)
        refused(blob, ptr, trace.size, 6)
        refused(blob, ptr, 0, 0)                                   # logn < 1
        refused(blob, ptr, int(blob[1]), 0)
        refused(blob, ptr, trace.size, -1)
        for n in (0, 1, 3, -1):                                    # n_stage2 not the program's
            refused(blob, ptr, trace.size, 5, n_stage2=n)
        at = 12 + int(blob[6]) + int(blob[7])                      # the stage-2 table
        for word, value in ((0, 0x5A), (at, 3), (at + 1, int(blob[1])), (at + 7, 1 << 40), (9, 33), (2, 11)):
            bad = blob.copy()
            bad[word] = value
            refused(bad, ptr, trace.size, 5)
        refused(blob[:-1], ptr, trace.size, 5)
        refused(blob[:11], ptr, trace.size, 5)
    finally:
        release()


def test_refusals():
    check_refusals(None, lambda arr: (np.ascontiguousarray(arr).ctypes.data, lambda: None))
    _, blob, trace, _ = WC.honest_case("chunk16", 5)
    with pytest.raises(native.ZpError):
        native.diagnose_stage2_host(blob, trace, 4)
    assert native.diagnose_stage2_host(WC.honest_case("fib", 5)[1], WC.honest_case("fib", 5)[2], 5) == []


def test_record_type():
    blob, trace, row = SC.case("broken_lookup", 5)
    perm, look = native.diagnose_stage2_host(blob, trace, 5)
    assert perm.ok and perm.kind == 1 and perm.row_a is None and perm.row_b is None and str(perm) == "permutation holds"
    assert not look.ok and look.verdict == native.S2_FAILS and (look.row_a, look.lhs_a, look.rhs_a) == (row, 1, 0)
    assert look.words == SC.expected(blob, trace, 5)[1] and "a row %d holds %d" % (row, look.value_a) in str(look)


def agree_with_the_check(check, diag, logn):
    """some record FAILS exactly when zp_stark_check_witness says VIOLATED, at a derived and at an explicit challenge"""
    cases = [WC.honest_case(n, logn)[1:] for n in ("perm", "chunk16")] + [WC.broken_perm(logn), WC.broken_lookup(logn)]
    for k, (blob, trace, pubs) in enumerate(cases):
        fails = any(rec[0] == SC.FAILS for rec in diag(blob, trace, logn))
        assert fails == (k >= 2)
        for chal in (None, WC.EXPLICIT_CHALLENGE):
            assert (check(blob, trace, pubs, logn, chal)[0][0] == WC.VIOLATED) == fails


@pytest.mark.parametrize("logn", [5, 9])
def test_consistent_with_the_witness_check(logn):
    from test_witness_check_host import host_check
    agree_with_the_check(host_check, host_diag, logn)


# ---- the engine: EngineConfig(check_witness=True, diagnose_stage2=True) on the tests' CPU backend
@pytest.fixture()
def cpu_factory(tables):
    from cpu_wrap_backend import CpuWrapBackend
    return lambda hash_mode="gl": CpuWrapBackend(*tables, hash_mode=hash_mode, bn_tables=None)


def engine_refusal(factory, monkeypatch, logn, **kw):
    """the WitnessError of a chunk whose range value at one row was put outside the table (WC.broken_lookup's edit on the engine's own witness),
    with the edited row"""
    from eigen_zeth_amd.service.engine import Engine, EngineConfig, WitnessError
    from eigen_zeth_amd.stark import air as AIR
    eng = Engine(factory, EngineConfig(air="chunk16", logn=logn, n_queries=2 if logn < 8 else 6, fri_final_log=3, pow_bits=4, chunks_per_block=1,
                                       prover_streams=2, **kw))
    ch = eng.gen_batch_chunks("b", [3], 12345, "evm")
    air = AIR.get_air("chunk16")
    Ww = air.width - 8
    fa, fb, r, q, tt, c, d = Ww, Ww + 1, Ww + 2, Ww + 3, Ww + 4, Ww + 6, Ww + 7
    seen = {}
    real = getattr(Engine._chunk_witness, "real", Engine._chunk_witness)       # a second call in one test patches the generator itself again

    def corrupted(a, chunk, out=None):
        t, pubs = real(a, chunk, out)
        # the first row from 5 on whose range value stands in no earlier row: the value taken out is then unbalanced only behind the edited row
        row = seen["row"] = next(i for i in range(5, t.shape[-1]) if not (t[r, :i] == t[r, i]).any())
        old, new = int(t[r, row]), int(max(int(v) for v in t[tt])) + 9
        t[r, row] = new
        t[q, int(np.nonzero(t[q] == np.uint64(old))[0][0])] = new
        t[c, row] = new * new % P
        t[d, row] = (int(t[fa, row]) * new + int(t[fb, row])) % P
        return t, pubs
    corrupted.real = real
    monkeypatch.setattr(Engine, "_chunk_witness", staticmethod(corrupted))
    with pytest.raises(WitnessError) as e:
        eng.gen_chunk_proofs("b", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    plan = json.loads(ch["batch_data"])["chunks"][0]
    return e.value, seen["row"], corrupted(air, plan)[0], eng


def check_engine_error(err, row, trace, diagnosed):
    N = trace.shape[-1]
    assert err.report.first_row == N - 1                 # what the check alone says: where the sum fails to close
    assert str(err) == str(err.report) and str(err).startswith("witness violates constraint %d at row %d (" % (err.report.first_constraint, N - 1))
    if not diagnosed:
        assert err.stage2 is None
        return
    perm, look = err.stage2
    from eigen_zeth_amd.stark import air as AIR
    blob = np.asarray(AIR.get_air("chunk16").program(), dtype=np.uint64)
    assert [perm.words, look.words] == SC.expected(blob, trace, N.bit_length() - 1)
    # two values: the one put in, and the one taken out, whose multiplicity is now one too many
    assert perm.ok and not look.ok and (look.row_a, look.lhs_a, look.rhs_a, look.unbalanced) == (row, 1, 0, 2)


def test_engine_names_the_row(cpu_factory, monkeypatch):
    err, row, trace, eng = engine_refusal(cpu_factory, monkeypatch, 5, check_witness=True, diagnose_stage2=True)
    check_engine_error(err, row, trace, True)
    err_off, row, trace, _ = engine_refusal(cpu_factory, monkeypatch, 5, check_witness=True)
    check_engine_error(err_off, row, trace, False)
    assert str(err_off) == str(err)
