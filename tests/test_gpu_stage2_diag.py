"""zp_stark_diagnose_stage2 on a ctx (csrc/stage2_diag.hip: s2_insert_kernel, s2_compare_kernel, s2_record_kernel over a hash table in HBM): every
record equals the host path's (ctx = NULL) and the multiset comparison of tests/stage2_diag_cases.py word for word -- exact integers -- at N = 2
(logn 1), less than a wave (5), one wave (6), two workgroups (9), sixteen (12) and, once, 2^16 rows with 2^17 keys (the grid, long probe runs); with
the wave's merge of equal keys ("s2_diag_merge") on and off."""
import numpy as np
import pytest

import stage2_diag_cases as SC
import witness_cases as WC
from test_stage2_diag_host import agree_with_the_check, check_engine_error, check_refusals, check_semantics, engine_refusal, host_diag, raw_diag
from eigen_zeth_amd import native

pytestmark = pytest.mark.gpu


def device_diag(prover, blob, trace, logn):
    """the records through the ctx; the trace must come back unchanged"""
    tr = np.ascontiguousarray(trace, dtype=np.uint64)
    d = prover.upload(tr)
    try:
        rc, recs = raw_diag(prover.ctx, blob, d.ptr, tr.size, logn)
        assert rc == 0, prover.lib.zp_last_error(prover.ctx)
        assert (prover.download(d, tr.shape) == tr).all()
    finally:
        d.free()
    return recs


@pytest.mark.parametrize("logn", sorted({l for _, l in SC.all_cases()}))
def test_records_equal_host_and_expectation(prover, logn):
    try:
        for merge in (1, 0):
            prover.set_tuning("s2_diag_merge", merge)
            for name in [n for n, l in SC.all_cases() if l == logn]:
                blob, trace, _ = SC.case(name, logn)
                want = SC.expected(blob, trace, logn)
                assert host_diag(blob, trace, logn) == want, name
                assert device_diag(prover, blob, trace, logn) == want, (name, merge)
    finally:
        prover.set_tuning("s2_diag_merge", 1)


@pytest.mark.parametrize("logn", SC.LOGNS)
def test_what_the_cases_mean(prover, logn):
    check_semantics(lambda blob, trace, lg: device_diag(prover, blob, trace, lg), logn)


def test_refusals_and_the_binding(prover):
    def ptr_of(arr):
        d = prover.upload(np.ascontiguousarray(arr, dtype=np.uint64))
        return d.ptr, d.free
    check_refusals(prover.ctx, ptr_of)
    blob, trace, row = SC.case("broken_lookup", 5)
    d = prover.upload(np.ascontiguousarray(trace))
    try:
        with pytest.raises(native.ZpError):
            prover.diagnose_stage2(blob, d, 4)
        perm, look = prover.diagnose_stage2(blob, d, 5)            # the ctx still works
        assert [perm.words, look.words] == SC.expected(blob, trace, 5) and perm.ok and (look.row_a, look.lhs_a, look.rhs_a) == (row, 1, 0)
    finally:
        d.free()


def test_consistent_with_the_witness_check(prover):
    from test_gpu_witness_check import device_check
    agree_with_the_check(lambda *a: device_check(prover, *a), lambda *a: device_diag(prover, *a), 9)


@pytest.mark.parametrize("check", [True, "prove"])
def test_engine_names_the_row_on_the_hip_backend(monkeypatch, check):
    """both paths to a WitnessError: the separate check, and the proof that checks itself (the prover only read the trace)"""
    from eigen_zeth_amd.service.server import default_backend_factory
    err, row, trace, _ = engine_refusal(default_backend_factory(0), monkeypatch, 8, check_witness=check, diagnose_stage2=True)
    check_engine_error(err, row, trace, True)
    err_off, row, trace, _ = engine_refusal(default_backend_factory(0), monkeypatch, 8, check_witness=check)
    check_engine_error(err_off, row, trace, False)
    assert str(err_off) == str(err)
