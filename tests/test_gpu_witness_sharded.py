"""The witness check over the ranks of a communicator (csrc/witness_sharded.hip): zp_stark_check_witness_sharded, the sharded provers under
"prove_check", and the row-window kernels they judge their rows with (csrc/witness_check.hip: witness_program_kernel<true>; stark/air.py:
emit_witness_rows_source -> `<symbol>_witness_rows`).

Every expectation is the checker's own row walk (tests/witness_cases.py: oracle_report) and the single-GPU call on the WHOLE trace
(zp_stark_check_witness / zp_stark_prove on the session's ctx) -- never the sharded code.  Ranks are threads of this process
(test_gpu_sharded_native.run_ranks: one ctx each, an in-process communicator).  A rank thread only COLLECTS what the calls return; every
assertion runs afterwards on the main thread, so a failing expectation never leaves a peer waiting in a collective.

Sizes: N / G = 2 (the smallest window: one row and the halo's neighbour), 32 (less than a wave), 256 (one workgroup, the seam to the next
rank's), 128 and 512 in between; logn 2, 5, 8, 9 over 1, 2, 4, 8 ranks wherever N / G >= 2.  `periodic` has a fixed column of period 8, so on 4
rows the statement does not exist: its smallest size, logn 3, is checked instead (as tests/test_gpu_witness_inproof.py does on 2 rows)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import witness_cases as WC
from test_gpu_sharded_native import run_ranks
from test_gpu_witness_inproof import ARGS, LOGN, raw_prove, raw_report, recorded_challenge, stages_of
from test_witness_check_host import raw_check
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR

pytestmark = pytest.mark.gpu

P, NONE = WC.P, WC.NONE
GEN, INTERP, EXCHANGE, CANON = "witness_program_rows_gen", "witness_program_rows", "witness_exchange", "witness_canonical"
PROGRAM_STAGES = {GEN, INTERP, "witness_program_gen", "witness_program"}
OK_REPORT = [WC.SATISFIED, NONE, NONE, 0, 0, 0, NONE, NONE]
_u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def hip(prover):
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    return HipBackend(prover=prover)


def raw_check_sharded(comm, blob, d_local, words, pubs, logn, chal=None):
    """the C call itself: (rc, report[8], counts[K], first_rows[K]), the outputs pre-filled by a pattern"""
    K = int(blob[8])
    pb = np.array([int(v) for v in pubs] + [0], dtype=np.uint64)
    ch = None if chal is None else np.array([int(v) for v in chal], dtype=np.uint64)
    rep, counts, first = (np.full(n, 0xA5A5A5A5, dtype=np.uint64) for n in (8, max(K, 1), max(K, 1)))
    p = lambda a: a.ctypes.data_as(_u64p)
    rc = comm.prover.lib.zp_stark_check_witness_sharded(comm.h, p(blob), blob.size, None if d_local is None else d_local.ptr, words, p(pb), len(pubs), logn,
                                                        None if ch is None else p(ch), p(rep), p(counts), p(first), K)
    return rc, [int(v) for v in rep], [int(v) for v in counts[:K]], [int(v) for v in first[:K]]


def my_slice(c, trace):
    first, count = c.my_columns(trace.shape[0])
    return np.ascontiguousarray(trace[first:first + count]) if count else None


def check_over_ranks(G, blob, rows_fn, cases, pubs, logn):
    """every (trace, challenge) of `cases` through zp_stark_check_witness_sharded on G ranks, generated kernel and interpreter:
    out[rank][case][knob] = ((rc, report, counts, first rows), stages, the rank holds columns)"""
    def fn(r, p, c):
        p.set_air_kernel_witness_rows(blob, rows_fn)
        out = []
        for trace, chal in cases:
            mine = my_slice(c, trace)
            d = p.upload(mine) if mine is not None else None
            got = {}
            for knob in (1, 0):
                p.set_tuning("witness_kernel", knob)
                got[knob] = stages_of(p, lambda: raw_check_sharded(c, blob, d, 0 if d is None else mine.size, pubs, logn, chal)) + (d is not None,)
            got["unchanged"] = d is None or bool((p.download(d, mine.shape) == mine).all())          # only read
            if d is not None:
                d.free()
            out.append(got)
        return out
    return run_ranks(G, fn)


def assert_reports(res, G, wants):
    for r in range(G):
        for got, want in zip(res[r], wants):
            assert got["unchanged"]
            for knob, ran, other in ((1, GEN, INTERP), (0, INTERP, GEN)):
                (rc, rep, counts, first), stages, has_cols = got[knob]
                assert rc == 0 and (rep, counts, first) == want, (r, knob, rep, want[0])
                assert (CANON in stages) == has_cols
                if want[0][0] == WC.NONCANONICAL:
                    assert EXCHANGE not in stages and not PROGRAM_STAGES & set(stages), stages
                else:
                    assert ran in stages and other not in stages and (EXCHANGE in stages) == (G > 1), (knob, stages)
                    assert not {"witness_program_gen", "witness_program"} & set(stages)


@functools.lru_cache(maxsize=None)
def wanted(name, logn, kind, chal=None):
    """(trace, the oracle's report) of one named trace"""
    air, blob, trace, pubs = WC.honest_case(name, logn)
    if kind == "honest":
        tr = trace
    elif kind == "perm":
        tr = WC.broken_perm(logn)[1]
    elif kind == "lookup":
        tr = WC.broken_lookup(logn)[1]
    else:
        tr = WC.flipped(trace, *kind)
    tr = np.ascontiguousarray(tr, dtype=np.uint64)
    return tr, WC.oracle_report(blob, tr, pubs, logn, list(chal) if chal else None)


@functools.lru_cache(maxsize=None)
def expectation(prover, name, logn, kind, chal=None):
    """... which the single-GPU call on the whole trace must already give"""
    _, blob, _, pubs = WC.honest_case(name, logn)
    tr, want = wanted(name, logn, kind, chal)
    d = prover.upload(tr)
    try:
        rc, rep, counts, first = raw_check(prover.ctx, blob, d.ptr, tr.size, pubs, logn, list(chal) if chal else None)
    finally:
        d.free()
    assert rc == 0 and (rep, counts, first) == want
    return tr, want


def window_cases(name, logn, G):
    """[(kind, challenge)] of the traces one (AIR, size, world) is checked on, after a look at what the oracle says of them"""
    N = 1 << logn
    nl = N // G
    air = WC.honest_case(name, logn)[0]
    W = air.width
    kinds = [("honest", None), ((0, 0), None), ((W - 1, N - 1), None)]          # row N - 1: the next row is rank 0's row 0
    inner = min(1, G - 1)                                                          # an inner rank's window (G = 2: the last; G = 1: the domain)
    kinds += [((0, inner * nl), None), ((W // 2, (inner + 1) * nl - 1), None)]     # its first and its last row
    if air.stage2:
        kinds.append(("honest", tuple(WC.EXPLICIT_CHALLENGE)))
    if name == "perm":
        kinds.append(("perm", None))
    if name == "chunk16":
        kinds += [("lookup", None), ("lookup", tuple(WC.EXPLICIT_CHALLENGE))]
    wants = [wanted(name, logn, kind, chal)[1] for kind, chal in kinds]
    assert wants[0] == (OK_REPORT, [0] * len(wants[0][1]), [NONE] * len(wants[0][1]))
    assert all(w[0][0] == WC.VIOLATED for (k, _), w in zip(kinds, wants) if k != "honest")
    for (k, _), w in zip(kinds, wants):
        if k in ("perm", "lookup"):
            assert w[0][1] == N - 1                    # the wrap-around row of a stage-2 constraint: judged by the LAST rank through rank 0's first row
    if G > 1 and name != "perm":
        # a flip on a window's first row is first seen by the row before it: on the PREVIOUS rank, through its halo (perm reads no trace column at
        # the next row; its broken permutation, a cell at row 3, shows at the wrap-around row of the last rank instead)
        assert wants[3][0][1] == inner * nl - 1
    return kinds


# ---------------------------------------------------------------------------------------------- the check before the proof, over the ranks
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("name", WC.SATISFIED_AIRS)
def test_check_over_the_ranks_equals_the_single_gpu_report(prover, hip, name, G):
    for logn in (2, 5, 8, 9):
        if name == "periodic" and logn == 2:
            logn = 3
        N = 1 << logn
        if N // G < 2:
            continue
        air, blob, trace, pubs = WC.honest_case(name, logn)
        kinds = window_cases(name, logn, G)
        made = [expectation(prover, name, logn, kind, chal) for kind, chal in kinds]
        wants = [w for _, w in made]
        res = check_over_ranks(G, blob, hip._airlib_witness_rows(air), [(tr, list(chal) if chal else None) for (tr, _), (_, chal) in zip(made, kinds)], pubs, logn)
        assert_reports(res, G, wants)


@pytest.mark.parametrize("logn", [5, 10])
def test_exact_counts_on_a_random_trace_over_four_ranks(prover, hip, logn):
    """chunk16's program over a seeded random canonical trace: nearly every row violates nearly every constraint; the merged counts are the oracle's
    integers -- four windows of 8 rows (the dead-lane mask) and of 256"""
    air, blob, _, _ = WC.honest_case("chunk16", logn)
    trace, pubs = WC.random_inputs(dict(width=air.width, n_pub=air.n_pub), logn, 7001 + logn)
    want = WC.oracle_report(blob, trace, pubs, logn)
    N = 1 << logn
    assert want[0][0] == WC.VIOLATED and want[0][3] == sum(want[1]) and sum(c >= N - 1 for c in want[1]) >= 8
    d = prover.upload(np.ascontiguousarray(trace))
    assert raw_check(prover.ctx, blob, d.ptr, trace.size, pubs, logn)[1:] == want
    d.free()
    assert_reports(check_over_ranks(4, blob, hip._airlib_witness_rows(air), [(trace, None)], pubs, logn), 4, [want])


def test_columns_that_do_not_divide(prover, hip):
    """the periodic AIR's 3 columns over 2 ranks (2 + 1) and over 4 (1 + 1 + 1 + 0: the last rank passes NULL)"""
    logn = 8
    air, blob, trace, pubs = WC.honest_case("periodic", logn)
    assert air.width == 3
    kinds = ["honest", (2, 7), (0, 128), (1, 255)]
    made = [expectation(prover, "periodic", logn, k) for k in kinds]
    assert [w[0][0] for _, w in made] == [WC.SATISFIED] + [WC.VIOLATED] * 3
    for G in (2, 4):
        res = check_over_ranks(G, blob, hip._airlib_witness_rows(air), [(tr, None) for tr, _ in made], pubs, logn)
        assert [res[r][0][1][2] for r in range(G)] == ([True, True] if G == 2 else [True, True, True, False])
        assert_reports(res, G, [w for _, w in made])


def test_noncanonical_words_are_reported_with_their_global_column(prover, hip):
    """one word = p in a column of the LAST rank that owns columns, a second in a lower rank's: count 2, the first in memory order, and nothing
    after the canonical pass on any rank"""
    logn = 8
    air, blob, trace, pubs = WC.honest_case("chunk16", logn)
    K = int(blob[8])
    bad = np.array(trace, dtype=np.uint64)
    bad[13, 5] = P               # rank 3 of 4 (columns 12..15), rank 1 of 2
    bad[6, 200] = P + 3          # rank 1 of 4, rank 0 of 2: the first in memory order
    want = ([WC.NONCANONICAL, NONE, NONE, 0, 0, 2, 6, 200], [0] * K, [NONE] * K)
    assert WC.oracle_report(blob, bad, pubs, logn) == want
    for G in (2, 4):
        assert_reports(check_over_ranks(G, blob, hip._airlib_witness_rows(air), [(bad, None)], pubs, logn), G, [want])
    air, blob, trace, pubs = WC.honest_case("periodic", logn)       # 1 + 1 + 1 + 0 columns: the last OWNER is rank 2
    K = int(blob[8])
    bad = np.array(trace, dtype=np.uint64)
    bad[2, 0] = P
    bad[1, 255] = 2 ** 64 - 1
    want = ([WC.NONCANONICAL, NONE, NONE, 0, 0, 2, 1, 255], [0] * K, [NONE] * K)
    assert WC.oracle_report(blob, bad, pubs, logn) == want
    assert_reports(check_over_ranks(4, blob, hip._airlib_witness_rows(air), [(bad, None)], pubs, logn), 4, [want])


def test_refusals_come_before_the_first_collective(prover):
    """fewer than two rows per rank, a wrong trace_words, a non-canonical public input: ZP_ERR_ARG on every rank, nobody waits, outputs untouched"""
    air, blob, trace, pubs = WC.honest_case("fib", 2)

    def fn(r, p, c):
        mine = my_slice(c, trace)
        d = p.upload(mine) if mine is not None else None
        return raw_check_sharded(c, blob, d, 0 if d is None else mine.size, pubs, 2)
    for out in run_ranks(4, fn):
        assert out[0] == -1 and out[1] == [0xA5A5A5A5] * 8

    for words_off, bad_pubs in ((1, pubs), (0, [P] + pubs[1:])):
        def fn(r, p, c):
            mine = my_slice(c, trace)
            return raw_check_sharded(c, blob, p.upload(mine), mine.size + words_off, bad_pubs, 2)
        for out in run_ranks(2, fn):
            assert out[0] == -1 and out[1] == [0xA5A5A5A5] * 8


def test_another_airs_kernel_gives_another_report(prover, hip):
    """that the registered row-window kernel really runs: with wide8's kernel under chunk16's program (its 12 constraints over the first 8 columns,
    which chunk16's wide mix satisfies) a flip in column 12 goes unseen, while the interpreter reports it"""
    logn = 8
    air, blob, trace, pubs = WC.honest_case("chunk16", logn)
    tr, want = expectation(prover, "chunk16", logn, (12, 100))
    assert want[0][0] == WC.VIOLATED
    other = hip._airlib_witness_rows(AIR.get_air("wide8"))
    res = check_over_ranks(2, blob, other, [(tr, None)], pubs, logn)
    for r in range(2):
        (rc1, rep1, _, _), stages1, _ = res[r][0][1]
        (rc0, rep0, counts0, first0), _, _ = res[r][0][0]
        assert rc0 == 0 and (rep0, counts0, first0) == want
        assert GEN in stages1 and (rc1 != 0 or rep1 != rep0)


# ---------------------------------------------------------------------------------------------- the check in the sharded proof
def raw_prove_sharded(c, air, blob, d_local, words, pubs, bn=False):
    """the C call itself: (rc, text or None, zp_last_error)"""
    p = c.prover
    pb = np.array([int(v) for v in pubs] + [0], dtype=np.uint64)
    out, n = C.c_void_p(), C.c_size_t(0)
    head = (c.h, air.name.encode(), blob.ctypes.data, blob.size, None if d_local is None else d_local.ptr, words, pb.ctypes.data, len(pubs))
    if bn:
        rc = p.lib.zp_stark_prove_sharded_bn128(*head, *ARGS[:5], C.byref(out), C.byref(n))
    else:
        rc = p.lib.zp_stark_prove_sharded(*head, *ARGS, C.byref(out), C.byref(n))
    if rc != 0:
        return rc, None if out.value is None and n.value == 0 else "a text came back", (p.lib.zp_last_error(p.ctx) or b"").decode()
    try:
        return rc, C.string_at(out.value, n.value).decode(), ""
    finally:
        p.lib.zp_free_buffer(out)


_VERDICTS = {}


def single_gpu_verdicts(prover, tables, name):
    """what the single-GPU prover says of the honest trace and of every bad one, and the oracle at the recorded challenge: G-independent, made once"""
    if name not in _VERDICTS:
        _VERDICTS[name] = _single_gpu_verdicts(prover, tables, name)
    return _VERDICTS[name]


def _single_gpu_verdicts(prover, tables, name):
    air, blob, trace, pubs = WC.honest_case(name, LOGN)
    K, N = int(blob[8]), 1 << LOGN
    bads = [WC.flipped(trace, air.width // 2, N // 2 + 1), WC.flipped(trace, 0, N // 2)]      # the second: a window's first row over 2 and 4 ranks
    if name == "perm":
        bads.append(WC.broken_perm(LOGN)[1])
    if name == "chunk16":
        bads.append(WC.broken_lookup(LOGN)[1])
    tr = np.ascontiguousarray(trace)
    d = prover.upload(tr)
    try:
        prover.set_tuning("prove_check", 0)
        rc, plain, err = raw_prove(prover, air, blob, d, pubs)
        assert rc == 0, err
        honest_chal = recorded_challenge(air, tr, pubs, tables) or [0, 0, 0]
        prover.set_tuning("prove_check", 1)
        out = []
        for bad in bads:
            bad = np.ascontiguousarray(bad)
            chal = recorded_challenge(air, bad, pubs, tables)
            want = WC.oracle_report(blob, bad, pubs, LOGN, chal)
            assert want[0][0] == WC.VIOLATED
            prover.h2d(d, bad)
            rc, text, err = raw_prove(prover, air, blob, d, pubs)
            assert rc == -7 and text is None and "constraint %d at row %d" % (want[0][2], want[0][1]) in err
            assert raw_report(prover, K) == (0, want[0], chal or [0, 0, 0], want[1], want[2])
            out.append((bad, err, raw_report(prover, K)))
    finally:
        prover.set_tuning("prove_check", 0)
        d.free()
    return plain, honest_chal, out


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", ["chunk16", "perm", "fib", "periodic"])
def test_sharded_provers_refuse_a_false_witness(prover, hip, tables, name, G):
    """THE test that fails without the feature: the parent returns a text where -7 is expected"""
    plain, honest_chal, bads = single_gpu_verdicts(prover, tables, name)
    air, blob, trace, pubs = WC.honest_case(name, LOGN)
    K = int(blob[8])
    rows_fn = hip._airlib_witness_rows(air)
    tr = np.ascontiguousarray(trace)

    def fn(r, p, c):
        p.set_air_kernel_witness_rows(blob, rows_fn)
        mine = my_slice(c, tr)
        words = 0 if mine is None else mine.size
        d = p.upload(mine) if mine is not None else None
        d_bad = p.alloc(words) if words else None
        log = {}
        prove = lambda buf: raw_prove_sharded(c, air, blob, buf, words, pubs)
        p.set_tuning("prove_check", 0)
        log["off"] = prove(d)
        if words:
            p.h2d(d_bad, my_slice(c, bads[0][0]))
        log["off_bad"] = prove(d_bad)                                       # today's behaviour: a text no verifier accepts
        p.set_tuning("prove_check", 1)
        for knob in (1, 0):
            p.set_tuning("witness_kernel", knob)
            log["on", knob] = stages_of(p, lambda: prove(d)) + (raw_report(p, K),)
            for i, (bad, _, _) in enumerate(bads):
                if words:
                    p.h2d(d_bad, my_slice(c, bad))
                log["bad", knob, i] = stages_of(p, lambda: prove(d_bad)) + (raw_report(p, K),)
            log["again", knob] = prove(d)                                   # the comm and the ctxs stay usable: the same bytes
        log["unchanged"] = not words or bool((p.download(d, mine.shape) == mine).all())
        return log, words != 0
    for r, (log, has_cols) in enumerate(run_ranks(G, fn)):
        assert log["unchanged"]
        assert log["off"] == (0, plain, "")
        rc, text, _ = log["off_bad"]
        assert rc == 0 and text and text != plain
        for knob, ran, other in ((1, GEN, INTERP), (0, INTERP, GEN)):
            (rc, text, err), stages, rep = log["on", knob]
            assert rc == 0 and text == plain, err
            assert ran in stages and other not in stages and EXCHANGE in stages and (CANON in stages) == has_cols, stages
            assert rep == (0, OK_REPORT, honest_chal, [0] * K, [NONE] * K)
            for i, (_, want_err, want_rep) in enumerate(bads):
                (rc, text, err), stages, rep = log["bad", knob, i]
                assert rc == native.ZP_ERR_WITNESS == -7 and text is None, (r, i, rc)
                assert err == want_err and rep == want_rep                  # the single-GPU prover's line and report, which are the oracle's
                assert ran in stages and EXCHANGE in stages
                if not air.stage2:
                    assert "lde" not in stages, stages                      # refused before the first extension
            assert log["again", knob] == (0, plain, "")


def test_sharded_prover_refuses_noncanonical_words_before_anything_else(prover, hip):
    air, blob, trace, pubs = WC.honest_case("chunk16", LOGN)
    K = int(blob[8])
    bad = np.array(trace, dtype=np.uint64)
    bad[4, 77] = P
    bad[12, 3] = P

    def fn(r, p, c):
        mine = my_slice(c, bad)
        d = p.upload(mine)
        p.set_tuning("prove_check", 1)
        got = stages_of(p, lambda: raw_prove_sharded(c, air, blob, d, mine.size, pubs)) + (raw_report(p, K),)
        d2 = p.upload(my_slice(c, np.ascontiguousarray(trace)))
        return got, raw_prove_sharded(c, air, blob, d2, mine.size, pubs)[0]
    for ((rc, text, err), stages, rep), again in run_ranks(4, fn):
        assert rc == -7 and text is None and "2 trace word(s)" in err and "column 4 at row 77" in err
        assert CANON in stages and not ({"lde", EXCHANGE} | PROGRAM_STAGES) & set(stages), stages
        assert rep == (0, [WC.NONCANONICAL, NONE, NONE, 0, 0, 2, 4, 77], [0, 0, 0], [0] * K, [NONE] * K)
        assert again == 0                      # the communicator and the ctxs survive the refusal


def test_sharded_bn128_prover_checks_its_trace(hip):
    air, blob, trace, pubs = WC.honest_case("chunk64", LOGN)
    rows_fn = hip._airlib_witness_rows(air)
    tr, bad = np.ascontiguousarray(trace), np.ascontiguousarray(WC.flipped(trace, 9, 100))
    p1 = native.Prover(0)
    try:
        p1.install_poseidon_bn254(17)
        d = p1.upload(tr)
        rc, plain, err = raw_prove(p1, air, blob, d, pubs, bn=True)
        assert rc == 0, err
        d.free()
    finally:
        p1.close()

    def fn(r, p, c):
        p.install_poseidon_bn254(17)
        p.set_air_kernel_witness_rows(blob, rows_fn)
        mine = my_slice(c, tr)
        d = p.upload(mine)
        p.set_tuning("prove_check", 1)
        out = []
        for knob in (1, 0):
            p.set_tuning("witness_kernel", knob)
            out.append(stages_of(p, lambda: raw_prove_sharded(c, air, blob, d, mine.size, pubs, bn=True)))
        p.h2d(d, my_slice(c, bad))
        return out, raw_prove_sharded(c, air, blob, d, mine.size, pubs, bn=True)
    for out, refused in run_ranks(2, fn):
        for ((rc, text, err), stages), ran in zip(out, (GEN, INTERP)):
            assert rc == 0 and text == plain and ran in stages and EXCHANGE in stages, err
        assert refused[0] == -7 and refused[1] is None


# ---------------------------------------------------------------------------------------------- callers
def test_backend_sharded_prover_raises_witness_error(prover, hip, tables):
    """HipBackend.prove_native_sharded(check=True): what Engine(check_witness="prove", final_ranks > 1) calls for its final STARK (the engine's own
    path to it needs a whole aggregation and a wrap key: minutes, not seconds)"""
    from eigen_zeth_amd.stark import prover as PR
    plain, _, bads = single_gpu_verdicts(prover, tables, "chunk16")
    air, blob, trace, pubs = WC.honest_case("chunk16", LOGN)
    params = PR.StarkParams(*ARGS[:5], pow_bits=ARGS[5])
    bad, want_err, (_, rep, chal, counts, first) = bads[0]
    with pytest.raises(native.WitnessError) as e:
        hip.prove_native_sharded(air, bad, pubs, params, 2, check=True)
    assert str(e.value) == want_err and e.value.report.counts == counts and e.value.report.first_constraint == rep[2] and e.value.report.chal == chal
    assert hip.prove_native_sharded(air, np.ascontiguousarray(trace), pubs, params, 2, check=True)[0] == plain
    text = hip.prove_native_sharded(air, bad, pubs, params, 2)[0]            # unchecked again: the knob does not stick to the rank ctxs
    assert text and text != plain


def test_compiled_host_checks_in_a_world_of_one(tmp_path, prover):
    """host/prove_chunk --check-prove and --check with `rank 0 world 1 id-file`: the sharded entry points on RCCL"""
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

    def run(flag, tr, name):
        np.ascontiguousarray(tr, dtype=np.uint64).tofile(tmp_path / "trace.bin")
        out = tmp_path / name
        r = subprocess.run([exe, flag, str(tmp_path / "program.bin"), str(tmp_path / "trace.bin"), str(tmp_path / "publics.bin"), str(logn), "1", "3", "3",
                            "6", "4", str(out), air.name, "0", "1", str(tmp_path / (name + ".id"))], capture_output=True, text=True, timeout=120)
        # RCCL prints its version banner on stdout when the communicator is made: the report is the one line that is a JSON object, and there is one
        reports = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(reports) == 1, r.stdout + r.stderr
        return r, out, json.loads(reports[0])["witness_check"]
    bad = WC.flipped(trace, 1, 100)                        # a wide-mix column: the verdict does not depend on the challenge
    want = WC.oracle_report(blob, bad, pubs, logn)
    for flag in ("--check-prove", "--check"):
        r, out, rep = run(flag, trace, "good.json")
        assert r.returncode == 0, r.stdout + r.stderr
        assert rep == {"verdict": "satisfied", "first_row": None, "first_constraint": None, "violations": 0, "violated_constraints": 0, "noncanonical": 0,
                       "first_noncanonical": None}
        assert out.read_text() == plain
        out.unlink()
        r, out, rep = run(flag, bad, "bad.json")
        assert r.returncode == 3 and not out.exists(), r.stdout + r.stderr
        assert (rep["verdict"], rep["first_row"], rep["first_constraint"], rep["violations"], rep["violated_constraints"]) == ("violated",) + tuple(want[0][1:5])
