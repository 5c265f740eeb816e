"""Random constraint programs through the GPU readers of the blob (-m gpu): the interpreter behind zp_eval_quotient /
zp_eval_quotient_rows (csrc/stark.hip: quotient_program_kernel) and zp_fixed_columns, on the case set of tests/program_cases.py --
blobs stark/air.py: compile_program would not have produced (every (opcode, kind, kind), 32 slots, 140 constraints, any operand
under OUT, arbitrary bits in the fields an OUT ignores).  The reference is the checker's C interpreter, which
tests/test_program_cases.py holds against the checker's Python reader on the same inputs.  Every comparison is exact."""
import numpy as np
import pytest

import program_cases as PC
from eigen_zeth_amd import native
from oracle import naive as NV
from oracle import oracle as O
from test_gpu_corner_data import corner_operands
from test_program_cases import (DOMAINS, NAMES, ROOT32, checker_quotient, checker_rows, decode, fold, inputs, planes_at, reference, refusal_base, w_last)

pytestmark = pytest.mark.gpu
P = O.P


def gpu_quotient(prover, blob, d, logm, logb, shift=49):
    M = 1 << logm
    d_cols, d_fixed, d_out = prover.upload(d["cols"]), prover.upload(d["fixed_dev"]), prover.alloc(3 * M)
    prover.eval_quotient(blob, d_cols, d_fixed, logm, logb, d["pubs"], d["apow"], d["zhinv"], shift, d["wlast"], d_out)
    got = prover.download(d_out, (3, M))
    for b in (d_cols, d_fixed, d_out):
        b.free()
    return got


@pytest.mark.parametrize("logm,logb", DOMAINS)
def test_interpreter_matches_the_checker_on_the_whole_domain(prover, logm, logb):
    for name in NAMES:
        blob, shape, d, ref = reference(name, logm, logb)
        assert (gpu_quotient(prover, blob, d, logm, logb) == ref).all(), name


def test_interpreter_on_corner_operands(prover):
    """every word the interpreter reads -- columns, fixed columns, public inputs, alpha powers, 1/Z_H -- drawn from the canonical corner
    operands (the carry and borrow classes of the field forms, tests/native/field_corners.hpp)"""
    ec = np.array([v for v in corner_operands() if v < P], dtype=np.uint64)
    draw = lambda shape, seed: np.ascontiguousarray(np.random.default_rng(seed).choice(ec, size=shape))
    logm, logb = 9, 1
    for name in ("cover", "slots32", "periods"):
        blob, shape = PC.case(name, logm - logb)
        d = inputs(shape, logm, logb, 0xC0DE, draw)
        assert (gpu_quotient(prover, blob, d, logm, logb) == checker_quotient(blob, d, logm, logb)).all(), name


@pytest.mark.parametrize("logb", [1, 2])
def test_row_windows_of_programs_with_periodic_columns(prover, logb):
    """zp_eval_quotient_rows with row0 != 0 on programs that read sparse columns of period 1, 4 and N: a window reads its periodic
    columns at (row0 + local row) mod the extended period.  Column, selector and output strides exceed nrows + blow-up."""
    logm = 10
    M, b = 1 << logm, 1 << logb
    periods_read = set()
    for name in PC.BOUNDED:
        blob, shape, d, ref = reference(name, logm, logb)
        assert sorted(shape["lp"]) == [0, 2, logm - logb]
        periods_read |= {shape["lp"][i - 2] for op, _, a, b_ in decode(blob)[0] for k, i in ((a,) if op == 4 else (a, b_)) if k == 3 and i >= 2}
        assert (gpu_quotient(prover, blob, d, logm, logb) == ref).all()
        periods = d["fixed_dev"][2 * M:]
        for row0, nrows in ((0, b), (M - b, b), (256, 320), (M // 2, M // 2), (3 * M // 4 - b, 2 * b)):
            sc, sf, so = nrows + b + 5, nrows + 3, nrows + 7
            cols = np.zeros((shape["width"], sc), dtype=np.uint64)
            cols[:, :nrows + b] = d["cols"][:, np.arange(row0, row0 + nrows + b) % M]
            fixed = np.zeros((2, sf), dtype=np.uint64)
            fixed[:, :nrows] = d["fixed_full"][:2, row0:row0 + nrows]
            d_cols, d_fixed, d_out = prover.upload(cols), prover.upload(np.concatenate([fixed.reshape(-1), periods])), prover.alloc(3 * so)
            prover.eval_quotient_rows(blob, d_cols, sc, d_fixed, sf, logm, logb, row0, nrows, d["pubs"], d["apow"], d["zhinv"], 49, d["wlast"], d_out, so)
            got = prover.download(d_out, (3, so))[:, :nrows]
            assert (got == ref[:, row0:row0 + nrows]).all(), (name, row0, nrows)
            rc, chk = checker_rows(blob, d, logm, logb, row0, nrows)
            assert rc == 0 and (got == chk).all(), (name, row0, nrows)
            for buf in (d_cols, d_fixed, d_out):
                buf.free()
    assert periods_read == {0, 2, logm - logb}


def fixed_columns_words(prover, blob, logn, logb):
    prog = np.ascontiguousarray(blob)
    return int(prover.lib.zp_fixed_columns_words(prog.ctypes.data, prog.size, logn, logb))


def fixed_columns_into(prover, blob, pubs, logn, logb, shift, d_out, out_words):
    """zp_fixed_columns with the caller's buffer size (Prover.fixed_columns sizes the buffer itself)"""
    prog = np.ascontiguousarray(blob)
    pb = np.array(list(pubs) + [0], dtype=np.uint64)
    prover._chk(prover.lib.zp_fixed_columns(prover.ctx, prog.ctypes.data, prog.size, pb.ctypes.data, len(pubs), logn, logb, shift, d_out.ptr, out_words))


ORDER8 = pow(ROOT32, 1 << 29, P)       # a coset shift of order 2^3: shift^(N/p) is 1 for the columns of period <= N/8 and not for the others


@pytest.mark.parametrize("logn,logb,lps,shift", [(1, 0, [0, 1], 49), (1, 0, [0, 1], 1), (4, 1, [0, 0, 2, 2, 2, 4], 49), (6, 2, [3, 1, 3, 6, 6], 49),
                                                 (9, 3, [0, 9], 49), (5, 0, [2, 5], 49), (5, 0, [2, 5], 1), (6, 0, [1, 3, 6], ORDER8)])
def test_fixed_columns_against_their_definition(prover, logn, logb, lps, shift):
    """zp_fixed_columns: sparse column k is the extension of the column tiled to N rows, of which one extended period is kept; the
    selectors are the extensions of the two indicator columns.  Columns: empty, every entry set, public entries only, values with p - 1
    (which column gets which walks with the shape).  shift 1 with blow-up 1 takes the plain-copy branch."""
    assert pow(ORDER8, 8, P) == 1 and pow(ORDER8, 4, P) != 1
    N, M = 1 << logn, 1 << (logn + logb)
    fills = [PC.FILLS[(i + logn) % 4] for i in range(len(lps))]
    blob, shape = PC.gen(300 + logn, logn, width=1, n_pub=5, n_const=1, n_slots=1, K=1, n_body=2, lps=lps, fills=fills)
    assert shape["lp"] == lps
    pubs = [P - 1] + [int(v) for v in O.random_field((4,), 310 + logn)]
    full = np.zeros((2 + len(lps), N), dtype=np.uint64)
    full[0, 0], full[1, N - 1] = 1, 1
    for k, (lp, ent) in enumerate(shape["sparse"]):
        period = np.zeros(1 << lp, dtype=np.uint64)
        for pos, is_pub, v in ent:
            period[pos] = pubs[v] if is_pub else v
        full[2 + k] = np.tile(period, N >> lp)
    ext = O.lde(full, logb, shift)
    want = np.concatenate([ext[0], ext[1]] + [ext[2 + k, :1 << (lp + logb)] for k, lp in enumerate(lps)])
    words = fixed_columns_words(prover, blob, logn, logb)
    assert words == len(want) == 2 * M + sum(1 << (lp + logb) for lp in lps)
    d_out = prover.alloc(words + 1)
    prover.h2d(d_out, np.full(words + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
    fixed_columns_into(prover, blob, pubs, logn, logb, shift, d_out, words)
    got = prover.download(d_out, (words + 1,))
    assert (got[:words] == want).all()
    assert int(got[words]) == 0x5A5A5A5A5A5A5A5A          # nothing behind the words it announced
    with pytest.raises(native.ZpError):
        fixed_columns_into(prover, blob, pubs, logn, logb, shift, d_out, words - 1)
    d_out.free()


@pytest.mark.parametrize("name", PC.BOUNDED)
def test_prover_and_verifier_read_a_random_statement_alike(prover, name):
    """Library functions only: the trace extended by zp_lde, the fixed columns from zp_fixed_columns, the planes sum_k alpha^k C_k from
    zp_eval_quotient (1/Z_H left out) -- interpolated and evaluated at zeta they must equal the same sum over zp_program_eval_ext's
    constraints at the columns' values from zp_ood_eval.  The cases keep every constraint below degree 4 N = M (3 (N - 1) + 2 < 4 N).
    What this catches and nothing else does: the prover's and the verifier's reading of a blob drifting apart together with a mirrored
    checker."""
    logn, logb, shift = 6, 2, 49
    N, M = 1 << logn, 1 << (logn + logb)
    blob, shape = PC.case(name, logn)
    W, seed = shape["width"], 9100 + NAMES.index(name)
    trace = O.random_field((W, N), seed)
    pubs = [int(v) for v in O.random_field((shape["n_pub"],), seed + 1)]
    alpha = [int(v) for v in O.random_field((3,), seed + 2)]
    zeta = [int(v) for v in O.random_field((3,), seed + 3)]
    apow = [[1, 0, 0]]
    for _ in range(shape["K"] - 1):
        apow.append(NV.e3_mul(apow[-1], alpha))
    d_ext = prover.alloc(W * M)
    prover.lde(prover.upload(trace), d_ext, logn, logb, W, shift)
    d_fixed = prover.fixed_columns(blob, pubs, logn, logb, shift)
    d_q = prover.alloc(3 * M)
    prover.eval_quotient(blob, d_ext, d_fixed, logn + logb, logb, pubs, apow, [1] * (1 << logb), shift, w_last(logn), d_q)
    lhs = planes_at(prover.download(d_q, (3, M)), zeta, shift)
    ev_z, ev_zw = prover.ood_eval(d_ext, M, 1 << logb, W, logn, shift, zeta, want_next=True)
    outs = native.program_eval_ext(blob, pubs, logn, ROOT32, zeta, ev_z, ev_zw)
    assert lhs == fold(outs, apow)


def test_thirty_two_slots_are_the_limit(prover):
    """a program with 32 slots that writes and reads slot 31 runs (64 KiB of LDS); one that announces 33 is refused"""
    logm, logb = 9, 1
    blob, shape, d, ref = reference("slots32", logm, logb)
    assert shape["n_slots"] == 32
    assert (gpu_quotient(prover, blob, d, logm, logb) == ref).all()
    bad = blob.copy()
    bad[9] = 33
    with pytest.raises(native.ZpError):
        gpu_quotient(prover, bad, d, logm, logb)


def test_malformed_programs_are_refused_before_anything_is_launched(prover):
    """the classes of tests/test_program_cases.py through zp_eval_quotient, the sparse-table ones through zp_fixed_columns too: each is
    ZP_ERR_ARG out of the validation in front of the launch.  Afterwards the ctx still evaluates a good program."""
    blob, shape, d = refusal_base()
    logm, logb = 6, 1
    want = checker_quotient(blob, d, logm, logb)
    assert (gpu_quotient(prover, blob, d, logm, logb) == want).all()
    classes = list(PC.malformed(blob, shape))
    const_p = blob.copy()
    const_p[12 + 2] = P                               # a word >= p in the table of constants
    classes.append(("constant_value_p", const_p))
    assert len(classes) == 21
    for cls, bad in classes:
        with pytest.raises(native.ZpError) as e:
            gpu_quotient(prover, bad, d, logm, logb)
        assert e.value.code == -1, cls
    words = fixed_columns_words(prover, blob, logm - logb, logb)
    d_out = prover.alloc(words)
    fixed_columns_into(prover, blob, d["pubs"], logm - logb, logb, 49, d_out, words)
    for cls, bad in PC.malformed_sparse(blob, shape):
        assert fixed_columns_words(prover, bad, logm - logb, logb) == 0, cls
        with pytest.raises(native.ZpError) as e:
            fixed_columns_into(prover, bad, d["pubs"], logm - logb, logb, 49, d_out, words)
        assert e.value.code == -1, cls
    d_out.free()
    assert (gpu_quotient(prover, blob, d, logm, logb) == want).all()


# ---- the acceptance table of csrc/air_program.hpp on the GPU readers: the variants of tests/test_program_readers.py.  Every variant is refused in
# front of the launch or runs a valid program: what zp_eval_quotient accepts of them differs from the good blob only in header words no kernel reads
# (Q, W with every operand in range, n_chal with a public-input vector to match, the stage-2 table), so its planes are the good blob's.
QUOTIENT_ACCEPTS = {("good", "plain"), ("good", "perm"), ("Q_0", "plain"), ("Q_17", "plain"), ("W_4096", "plain"), ("n_chal_1_no_stage2", "plain"),
                    ("Q_0", "perm"), ("Q_17", "perm"), ("W_4096", "perm"), ("stage2_kind_3", "perm"), ("stage2_column_W", "perm")}


def reader_variants(logn):
    """(name, base, blob) of tests/test_program_readers.py with the stage-2 program on 2^logn rows; bases: name -> (blob, trace, publics)"""
    import test_program_readers as TR
    import witness_cases as WC
    _, vs = TR.variants()
    _, perm, ptrace, ppubs = WC.honest_case("perm", logn)
    perm4 = WC.honest_case("perm", 4)[1]
    assert (perm == perm4).all()                          # the program does not depend on the trace length: the variants cut at 2^4 rows are its variants
    blob, shape, _ = refusal_base()
    trace, pubs = WC.random_inputs(shape, 5, 4100)
    return {"plain": (blob, trace, pubs), "perm": (perm, ptrace, ppubs)}, [v for v in vs if v[1] != "one_slot"]


def test_reader_variants_through_the_quotient_interpreter(prover):
    """zp_eval_quotient at (logm, logb) = (6, 1), one partial workgroup: accept or refuse per variant, and the accepted ones give the good blob's planes"""
    logm, logb = 6, 1
    bases, vs = reader_variants(5)
    good, seen = {}, set()
    for name, base, blob in vs:
        g = bases[base][0]
        shape = {"width": int(g[1]) + int(g[2]), "K": int(g[8]), "n_pub": int(g[4]) + int(g[5]), "lp": [l for l, _ in decode(g)[1]]}
        d = inputs(shape, logm, logb, 8900)
        d["pubs"] = d["pubs"] + [7] * (int(blob[4]) + int(blob[5]) - len(d["pubs"]))      # as many as the variant's header announces
        try:
            got = gpu_quotient(prover, blob, d, logm, logb)
        except native.ZpError as e:
            assert e.code == -1, (name, base)
            continue
        seen.add((name, base))
        if name == "good":
            good[base] = got
        assert (got == good[base]).all(), (name, base)
    assert seen == QUOTIENT_ACCEPTS
    blob, shape, d = refusal_base()
    assert (good["plain"] == checker_quotient(blob, inputs(shape, logm, logb, 8900), logm, logb)).all()


def test_reader_variants_through_the_device_witness_check(prover):
    """zp_stark_check_witness with a ctx on 2^5 rows: the witness check asks for every group, so only the good blobs are taken"""
    import witness_cases as WC
    bases, vs = reader_variants(5)
    for name, base, blob in vs:
        _, trace, pubs = bases[base]
        d_trace = prover.upload(np.ascontiguousarray(trace))
        chal = WC.EXPLICIT_CHALLENGE if int(blob[10]) else None
        if name == "good":
            rep = prover.check_witness(blob, d_trace, pubs, 5, chal)
            assert rep.ok == (base == "perm")             # perm's own witness; a random trace for the other
        else:
            with pytest.raises(native.ZpError) as e:
                prover.check_witness(blob, d_trace, pubs, 5, chal)
            assert e.value.code == -1, (name, base)
        d_trace.free()


def test_stage2_variants_through_the_prover(prover):
    """zp_stark_prove on 2^5 rows, blow-up 2: a stage-2 table with an unknown kind or a column outside the trace is refused by make_shape"""
    import witness_cases as WC
    bases, vs = reader_variants(5)
    blob, trace, pubs = bases["perm"]
    assert int(blob[11]) <= 2
    d_trace = prover.upload(np.ascontiguousarray(trace))
    assert prover.stark_prove("perm", blob, d_trace, pubs, 5, 1, 2, 3, 3, 0).startswith("{")
    for name, base, bad in vs:
        if name.startswith("stage2"):
            with pytest.raises(native.ZpError) as e:
                prover.stark_prove("perm", bad, d_trace, pubs, 5, 1, 2, 3, 3, 0)
            assert e.value.code == -1, name
    d_trace.free()
