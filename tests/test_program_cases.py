"""Random constraint programs (tests/program_cases.py) through the readers of the blob that need no GPU: the checker's C interpreter
(oracle/gl_oracle.c: orc_quotient_program), the checker's Python reader (oracle/air_program.py: Program) and the library's host
evaluator at the out-of-domain point (csrc/verify.hip: zp_program_eval_ext, zp_program_fixed_eval_ext).  Every comparison is exact.
The GPU interpreter and zp_fixed_columns meet the same blobs in tests/test_gpu_program_cases.py, which takes its inputs and its
reference from the helpers below."""
import numpy as np
import pytest

import program_cases as PC
from oracle import naive as NV
from oracle import oracle as O
from oracle.air_program import BadProgram, Program

P = O.P
ROOT32 = O.ROOT32_DEFAULT
# (logm, logb) of the whole-domain comparisons: M = 8 is one partial workgroup of the GPU interpreter, M = 256 exactly one; logb = 0 is
# blow-up 1; logb = logm a trace of one row
DOMAINS = [(3, 0), (3, 3), (8, 1), (9, 2), (12, 1), (12, 3)]
NAMES = [c[0] for c in PC.CASES]


def w_last(logn):
    """w_N^(N-1)"""
    return pow(NV.root(logn, ROOT32), (1 << logn) - 1, P) if logn else 1


def inputs(shape, logm, logb, seed, draw=O.random_field):
    """what one evaluation over the 2^logm-row domain reads.  The fixed columns are data laid out as the GPU interpreter reads them --
    two full columns, then ONE extended period of 2^(lp + logb) words per sparse column -- and, for the checker, the same data tiled to
    M rows.  draw(shape, seed) makes the words."""
    M, b = 1 << logm, 1 << logb
    d = {"cols": draw((shape["width"], M), seed), "apow": draw((shape["K"], 3), seed + 1), "zhinv": draw((b,), seed + 2),
         "pubs": [int(v) for v in draw((max(shape["n_pub"], 1),), seed + 3)][:shape["n_pub"]]}
    sel = draw((2, M), seed + 4)
    periods = [draw((1 << (lp + logb),), seed + 5 + k) for k, lp in enumerate(shape["lp"])]
    d["fixed_dev"] = np.concatenate([sel.reshape(-1)] + periods)
    d["fixed_full"] = np.ascontiguousarray(np.stack([sel[0], sel[1]] + [np.tile(p, M // len(p)) for p in periods]))
    d["wlast"] = w_last(logm - logb)
    return d


def checker_rows(blob, d, logm, logb, row0, nrows, shift=49):
    """orc_quotient_program_rows on the window [row0, row0 + nrows): (return code, planes [3][nrows]); the window carries its halo"""
    M, b = 1 << logm, 1 << logb
    whole = row0 == 0 and nrows == M
    rows = np.arange(row0, row0 + nrows + (0 if whole else b)) % M
    cols = np.ascontiguousarray(d["cols"][:, rows])
    fixed = np.ascontiguousarray(d["fixed_full"][:, row0:row0 + nrows])
    prog = np.ascontiguousarray(blob)
    out = np.zeros((3, nrows), dtype=np.uint64)
    pub = np.array(list(d["pubs"]) + [0], dtype=np.uint64)
    ap, zh = np.ascontiguousarray(d["apow"]).reshape(-1), np.ascontiguousarray(d["zhinv"])
    rc = O.lib().orc_quotient_program_rows(O._p(prog), prog.size, O._p(cols), cols.shape[1], O._p(fixed), fixed.shape[1], M, b, row0, nrows, O._p(pub),
                                           O._p(ap), O._p(zh), shift, NV.root(logm, ROOT32) if logm else 1, d["wlast"], O._p(out), nrows)
    return rc, out


def checker_quotient(blob, d, logm, logb, shift=49):
    """orc_quotient_program on the whole domain: planes [3][M]"""
    M = 1 << logm
    prog = np.ascontiguousarray(blob)
    out = np.zeros((3, M), dtype=np.uint64)
    pub = np.array(list(d["pubs"]) + [0], dtype=np.uint64)
    ap, zh = np.ascontiguousarray(d["apow"]).reshape(-1), np.ascontiguousarray(d["zhinv"])
    rc = O.lib().orc_quotient_program(O._p(prog), prog.size, O._p(d["cols"]), O._p(d["fixed_full"]), M, 1 << logb, O._p(pub), O._p(ap), O._p(zh), shift,
                                      NV.root(logm, ROOT32) if logm else 1, d["wlast"], O._p(out))
    assert rc == 0
    return out


_reference = {}


def reference(name, logm, logb):
    """(blob, shape, inputs, the checker's planes) of a case on a domain, computed once and left unchanged"""
    key = (name, logm, logb)
    if key not in _reference:
        blob, shape = PC.case(name, logm - logb)
        d = inputs(shape, logm, logb, 7000 + 100 * NAMES.index(name) + 10 * logm + logb)
        ref = checker_quotient(blob, d, logm, logb)
        for a in (blob, ref, d["cols"], d["fixed_dev"], d["fixed_full"]):
            a.setflags(write=False)
        _reference[key] = (blob, shape, d, ref)
    return _reference[key]


def python_row(prog, d, logm, logb, r, shift=49):
    """Program.evaluate_base on row r, folded as the interpreters fold it"""
    M, b = 1 << logm, 1 << logb
    x = shift * pow(NV.root(logm, ROOT32) if logm else 1, r, P) % P
    col = lambda rr: [int(v) for v in d["cols"][:, rr]]
    outs = prog.evaluate_base(col(r), col((r + b) % M), [int(v) for v in d["fixed_full"][:, r]], d["pubs"], (x - d["wlast"]) % P)
    zi = int(d["zhinv"][r % b])
    return [sum(o * int(d["apow"][k, c]) for k, o in enumerate(outs)) % P * zi % P for c in range(3)]


def selectors_at(zeta, logn):
    """L_first, L_last of the 2^logn-row trace domain at the F_{p^3} point zeta"""
    N, wl = 1 << logn, w_last(logn)
    zn = NV.e3_pow(zeta, N)
    zh = [(zn[0] - 1) % P * pow(N, P - 2, P) % P, zn[1] * pow(N, P - 2, P) % P, zn[2] * pow(N, P - 2, P) % P]
    first = NV.e3_mul(zh, NV.e3_inv([(zeta[0] - 1) % P, zeta[1], zeta[2]]))
    last = NV.e3_mul([v * wl % P for v in zh], NV.e3_inv([(zeta[0] - wl) % P, zeta[1], zeta[2]]))
    return first, last


def python_at_zeta(prog, pubs, logn, zeta, ev_z, ev_zw):
    """(fixed columns, constraints) at zeta from the checker's Python reader"""
    first, last = selectors_at(zeta, logn)
    fixed = [first, last] + [prog.fixed_eval_ext(k, pubs, zeta, logn, ROOT32) for k in range(len(prog.fixed_cols))]
    outs = prog.evaluate_ext([[int(v) for v in e] for e in ev_z], [[int(v) for v in e] for e in ev_zw], fixed, pubs,
                             [(zeta[0] - w_last(logn)) % P, zeta[1], zeta[2]])
    return fixed, outs


def fold(outs, apow):
    """sum_k apow[k] C_k in F_{p^3}"""
    acc = [0, 0, 0]
    for o, a in zip(outs, apow):
        acc = NV.e3_add(acc, NV.e3_mul([int(v) for v in o], [int(v) for v in a]))
    return acc


def planes_at(planes, zeta, shift):
    """the F_{p^3} value at zeta of the polynomial whose three coefficient planes are given by their values on shift <w_M>: plane c
    carries the coefficient of t^c"""
    sinv = pow(shift, P - 2, P)
    at = O.poly_eval_e3_cols(O.intt(planes), [v * sinv % P for v in zeta])
    acc = [0, 0, 0]
    for c, basis in enumerate(([1, 0, 0], [0, 1, 0], [0, 0, 1])):
        acc = NV.e3_add(acc, NV.e3_mul([int(v) for v in at[c]], basis))
    return acc


def decode(blob):
    """the instruction words of a blob as (op, dst, (kind a, index a), (kind b, index b)) and the sparse columns' (lp, entry words)"""
    w = [int(v) for v in blob]
    n_const, n_instr = w[6], w[7]
    ins = [(x & 0xFF, (x >> 8) & 0xFFFF, ((x >> 24) & 0xF, (x >> 28) & 0xFFFF), ((x >> 44) & 0xF, (x >> 48) & 0xFFFF)) for x in w[12 + n_const:12 + n_const + n_instr]]
    at, cols = 12 + n_const + n_instr + 4 * w[10], []
    for _ in range(w[3] - 2):
        lp, ne = w[at] & 0xFF, w[at] >> 8
        cols.append((lp, w[at + 1:at + 1 + 2 * ne]))
        at += 1 + 2 * ne
    assert at == len(w)
    return ins, cols


def test_case_set_covers_the_grammar():
    """the conditions the case set exists for, read off the blobs by bit arithmetic; and the checker's reader accepts every case"""
    triples, out_kinds, slot_counts, Ks, n_consts, lp_lists = set(), set(), set(), set(), set(), []
    max_pub, out_dst, out_kb, xml_a = 0, set(), set(), False
    for name in NAMES:
        blob, shape = PC.case(name, 7)
        hdr = [int(v) for v in blob[:12]]
        assert hdr[0] == PC.MAGIC and hdr[2] == 0 and hdr[5] == 0 and hdr[10] == 0
        assert (hdr[1], hdr[3], hdr[4], hdr[6], hdr[7], hdr[8], hdr[9]) == (shape["width"], shape["n_fixed"], shape["n_pub"], shape["n_const"], shape["n_instr"],
                                                                           shape["K"], shape["n_slots"])
        assert all(int(v) < P for v in blob[12:12 + hdr[6]])
        ins, cols = decode(blob)
        limit = [hdr[9], hdr[1], hdr[1], hdr[3], hdr[4], hdr[6], 1]
        written, read = set(), set()
        for op, dst, a, b in ins:
            assert 1 <= op <= 4
            for kind, idx in ((a,) if op == 4 else (a, b)):
                assert kind <= 6 and idx < limit[kind]
                if kind == 0:
                    assert idx in written, "a slot is read before it is written"
                    read.add(idx)
                if kind == 4:
                    max_pub = max(max_pub, idx)
            if op == 4:
                out_kinds.add(a[0])
                out_dst.add(dst)
                out_kb.add(b[0])
            else:
                assert dst < hdr[9]
                written.add(dst)
                triples.add((op, a[0], b[0]))
                xml_a |= a[0] == 6
        assert sum(op == 4 for op, _, _, _ in ins) == hdr[8]
        if hdr[9] == 32:
            assert 31 in written and 31 in read
        for lp, ent in cols:
            assert len(ent) // 2 <= 1 << lp and len({e & ~(1 << 63) for e in ent[0::2]}) == len(ent) // 2
            for pos, v in zip(ent[0::2], ent[1::2]):
                assert pos & ~(1 << 63) < 1 << lp and (v < hdr[4] if pos >> 63 else v < P)
        slot_counts.add(hdr[9])
        Ks.add(hdr[8])
        n_consts.add(hdr[6])
        lp_lists.append([lp for lp, _ in cols])
        assert lp_lists[-1] == shape["lp"]
        Program(blob)
        for logn in (0, 3):                      # the clamped forms the small domains use
            Program(PC.case(name, logn)[0])
    assert triples == {(op, ka, kb) for op in (1, 2, 3) for ka in range(7) for kb in range(7)} and len(triples) == 147
    assert out_kinds == set(range(7))
    assert {1, 8, 32} <= slot_counts
    assert max(Ks) >= 130 and 1 in Ks
    assert 0 in n_consts and max(n_consts) >= 40
    assert max_pub >= 16
    assert xml_a                                  # x - w_last as the FIRST operand
    assert len(out_dst) > 20 and any(k > 6 for k in out_kb)      # the ignored fields of an OUT hold arbitrary bits
    flat = {lp for l in lp_lists for lp in l}
    assert {0, 1, 7} <= flat
    assert any(l[i] == l[i + 1] == l[i + 2] for l in lp_lists for i in range(len(l) - 2))
    assert any(l[i] == l[i + 2] != l[i + 1] for l in lp_lists for i in range(len(l) - 2))
    fills = {(len(ent) // 2 == 0, len(ent) // 2 == 1 << lp, bool(ent) and all(e >> 63 for e in ent[0::2]))
             for name in NAMES for lp, ent in decode(PC.case(name, 7)[0])[1]}
    assert (True, False, False) in fills and (False, True, False) in fills and (False, True, True) in fills     # empty, full, public entries only


@pytest.mark.parametrize("name", PC.BOUNDED)
def test_bounded_cases_keep_their_degree_bound(name):
    """the degree of every slot, recomputed from the words as stark/air.py: degree counts it (componentwise), stays within a = 3, b = 2"""
    ins, _ = decode(PC.case(name, 6)[0])
    leaf = {1: (1, 0), 2: (1, 0), 3: (1, 0), 4: (0, 0), 5: (0, 0), 6: (0, 1)}
    deg = {}
    for op, dst, a, b in ins:
        if op == 4:
            continue
        da, db = [deg[i] if k == 0 else leaf[k] for k, i in (a, b)]
        deg[dst] = (da[0] + db[0], da[1] + db[1]) if op == 3 else (max(da[0], db[0]), max(da[1], db[1]))
        assert deg[dst][0] <= 3 and deg[dst][1] <= 2


@pytest.mark.parametrize("logm,logb", [(3, 0), (3, 3), (7, 1), (9, 2), (12, 3)])
def test_c_interpreter_matches_the_python_reader(logm, logb):
    """orc_quotient_program against Program.evaluate_base: every row up to 2^7 rows, a seeded sample of 64 rows above.  The C interpreter
    is then the reference for all rows (the GPU tests compare with it)"""
    M = 1 << logm
    for name in NAMES:
        blob, shape, d, ref = reference(name, logm, logb)
        prog = Program(blob)
        rows = range(M) if logm <= 7 else sorted({0, M - 1, M - (1 << logb)} | set(np.random.default_rng(logm).choice(M, 64, replace=False).tolist()))
        for r in rows:
            assert python_row(prog, d, logm, logb, r) == [int(v) for v in ref[:, r]], (name, r)


@pytest.mark.parametrize("logm,logb", [(6, 1), (10, 2)])
def test_c_interpreter_row_windows_match_the_whole_domain(logm, logb):
    M, b = 1 << logm, 1 << logb
    for name in NAMES:
        blob, shape, d, ref = reference(name, logm, logb)
        for row0, nrows in ((0, b), (M - b, b), (M // 2, M // 2), (3 * M // 4 - b, 2 * b)):
            rc, got = checker_rows(blob, d, logm, logb, row0, nrows)
            assert rc == 0 and (got == ref[:, row0:row0 + nrows]).all(), (name, row0)


@pytest.mark.parametrize("logn", [3, 4, 5, 6])
def test_host_evaluator_at_zeta_matches_the_python_reader(logn):
    """zp_program_eval_ext / zp_program_fixed_eval_ext against Program.evaluate_ext / fixed_eval_ext on every case (periods 1 .. N)"""
    from eigen_zeth_amd import native
    for i, name in enumerate(NAMES):
        blob, shape = PC.case(name, logn)
        prog = Program(blob)
        pubs = [int(v) for v in O.random_field((shape["n_pub"] + 1,), 8100 + i)][:shape["n_pub"]]
        ev_z, ev_zw = O.random_field((shape["width"], 3), 8200 + i), O.random_field((shape["width"], 3), 8300 + i)
        for zeta in ([int(v) for v in O.random_field((3,), 8400 + 10 * i + logn)], [12345, 0, 0]):
            fixed, outs = python_at_zeta(prog, pubs, logn, zeta, ev_z, ev_zw)
            assert native.program_fixed_eval_ext(blob, pubs, logn, ROOT32, zeta).tolist() == fixed, name
            assert native.program_eval_ext(blob, pubs, logn, ROOT32, zeta, ev_z, ev_zw).tolist() == outs, name


def checker_statement(name, logn, logb, shift=49):
    """a random 'statement' of a degree-bounded case: trace, public inputs, alpha powers, and -- all from the checker -- the extended
    columns, the materialised fixed columns and the planes sum_k alpha^k C_k on the coset (1/Z_H left out: zhinv = 1)"""
    blob, shape = PC.case(name, logn)
    seed = 9000 + 10 * NAMES.index(name) + logn
    N, M = 1 << logn, 1 << (logn + logb)
    trace = O.random_field((shape["width"], N), seed)
    pubs = [int(v) for v in O.random_field((shape["n_pub"],), seed + 1)]
    alpha = [int(v) for v in O.random_field((3,), seed + 2)]
    apow = [[1, 0, 0]]
    for _ in range(shape["K"] - 1):
        apow.append(NV.e3_mul(apow[-1], alpha))
    ind = np.zeros((2 + len(shape["lp"]), N), dtype=np.uint64)
    ind[0, 0], ind[1, N - 1] = 1, 1
    prog = Program(blob)
    for k in range(len(shape["lp"])):
        ind[2 + k] = np.tile(np.array(prog.fixed_period(k, pubs), dtype=np.uint64), N >> shape["lp"][k])
    d = {"cols": O.lde(trace, logb, shift), "fixed_full": O.lde(ind, logb, shift), "pubs": pubs, "apow": np.array(apow, dtype=np.uint64),
         "zhinv": np.ones(1 << logb, dtype=np.uint64), "wlast": w_last(logn)}
    return blob, shape, trace, d


@pytest.mark.parametrize("logn", [4, 6])
@pytest.mark.parametrize("name", PC.BOUNDED)
def test_planes_interpolate_to_the_constraints_at_zeta(name, logn):
    """The identity the GPU test asks of the library, with the checker in every role (this guards the test's own algebra): the planes
    sum_k alpha^k C_k on the coset are polynomials of degree < M = 4 N (the cases' degree bound: 3 (N - 1) + 2 < 4 N), so their
    interpolants at zeta equal the constraints evaluated from the columns' values at zeta and zeta w_N"""
    logb = 2
    blob, shape, trace, d = checker_statement(name, logn, logb)
    planes = checker_quotient(blob, d, logn + logb, logb)
    zeta = [int(v) for v in O.random_field((3,), 9500 + logn)]
    coef = O.intt(trace)
    ev_z = O.poly_eval_e3_cols(coef, zeta)
    ev_zw = O.poly_eval_e3_cols(coef, [v * NV.root(logn, ROOT32) % P for v in zeta])
    _, outs = python_at_zeta(Program(blob), d["pubs"], logn, zeta, ev_z, ev_zw)
    assert planes_at(planes, zeta, 49) == fold(outs, d["apow"])


def refusal_base():
    """the good blob the malformed ones are cut from, and its inputs on a 2^6-row domain"""
    blob, shape = PC.gen(110, 5, width=3, n_pub=4, n_const=5, n_slots=6, K=4, n_body=20, lps=(2, 1), fills=("full", "pub"))
    return blob, shape, inputs(shape, 6, 1, 8800)


def test_malformed_programs_are_refused_by_every_validating_reader():
    """One word of a good blob changed, per class.  Program and zp_program_eval_ext validate everything they read and must refuse every
    class.  The C interpreter is documented to check the magic, the length, opcodes and operand kinds only (it takes the sparse columns
    materialised and does not range-check indices): it is handed those classes alone."""
    from eigen_zeth_amd import native
    blob, shape, d = refusal_base()
    ev = O.random_field((shape["width"], 3), 8801)
    zeta = [int(v) for v in O.random_field((3,), 8802)]
    Program(blob)
    native.program_eval_ext(blob, d["pubs"], 5, ROOT32, zeta, ev, ev)
    assert checker_rows(blob, d, 6, 1, 0, 64)[0] == 0
    seen = set()
    for cls, bad in PC.malformed(blob, shape):
        seen.add(cls)
        with pytest.raises(BadProgram):
            Program(bad)
        with pytest.raises(ValueError):
            native.program_eval_ext(bad, d["pubs"], 5, ROOT32, zeta, ev, ev)
        if cls in SPARSE_CLASSES or cls.startswith("one_word"):      # what the fixed-column evaluator reads of a blob
            with pytest.raises(ValueError):
                native.program_fixed_eval_ext(bad, d["pubs"], 5, ROOT32, zeta)
        if cls.startswith(("opcode", "kind_7", "one_word")):
            assert checker_rows(bad, d, 6, 1, 0, 64)[0] == -1, cls
    assert len(seen) == 20 and SPARSE_CLASSES <= seen
    # (A word >= p in the table of CONSTANTS is a class of zp_eval_quotient alone -- tests/test_gpu_program_cases.py: zp_program_eval_ext
    # reads a constant mod p and the checker's readers do not look at the constants, by their own code; it is asserted of neither.)


SPARSE_CLASSES = {"entry_pos_at_period", "public_entry_pos_at_period", "public_entry_index_at_n_pub", "entry_value_p"}
