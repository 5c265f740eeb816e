"""Which reader of a ZPAIR1 constraint program takes which blob (no GPU): the acceptance table of csrc/air_program.hpp ("who asks for what"),
pinned cell by cell.  The readers differ on purpose or by history -- zp_program_eval_ext takes up to 2^16 slots, reads n_slots = 0 as one slot
and a constant >= p mod p, and never looks at Q or the stage-2 table; the witness check asks for everything -- and this table is what they did
when each had its own copy of the parsing code.  One word of a good blob is changed per variant (n_const = 2^16 also grows the blob to match),
and every entry point is called with ctx = NULL.  The public inputs and challenges are as many as the variant's header announces; the trace and
the evaluations keep the good blob's width, so for W_4096 zp_program_eval_ext and zp_stark_check_witness would refuse the array sizes as well:
only the fixed-column evaluators' cells pin the widths group there.  Everywhere else a refusal is the blob's.
Where zp_program_eval_ext accepts, its words are compared with oracle/air_program.py's Program if that reader takes the blob too."""
import numpy as np

import program_cases as PC
import witness_cases as WC
from oracle import oracle as O
from oracle.air_program import BadProgram, Program
from test_program_cases import ROOT32, refusal_base, selectors_at, w_last

P = O.P
READERS = ("eval_ext", "fixed_eval_ext", "fixed_eval_ext_batch", "check_witness", "fixed_columns_words")


def _bases():
    """name -> (blob, trace, publics, logn): a program without stage 2 and with sparse columns, a stage-2 program, and a one-slot program"""
    blob, shape, _ = refusal_base()
    trace, pubs = WC.random_inputs(shape, 5, 4100)
    _, perm, ptrace, ppubs = WC.honest_case("perm", 4)
    one, oshape = PC.case("one_slot_one_constraint", 4)
    otrace, opubs = WC.random_inputs(oshape, 4, 4101)
    return {"plain": (blob, trace, pubs, 5), "perm": (perm, ptrace, ppubs, 4), "one_slot": (one, otrace, opubs, 4)}


def _with(blob, at, v):
    b = np.array(blob, dtype=np.uint64)
    b[at] = v
    return b


def variants():
    """(name, base, blob)"""
    bases = _bases()
    plain, perm, one = bases["plain"][0], bases["perm"][0], bases["one_slot"][0]
    assert int(plain[10]) == 0 and int(plain[6]) >= 3 and int(perm[10]) >= 1 and int(perm[5]) == 3 and int(one[9]) == 1
    out = [("good", b, bases[b][0]) for b in bases]
    for base, blob in (("plain", plain), ("perm", perm)):
        out += [("n_slots_0", base, _with(blob, 9, 0)), ("n_slots_33", base, _with(blob, 9, 33)), ("n_slots_65537", base, _with(blob, 9, 65537)),
                ("Q_0", base, _with(blob, 11, 0)), ("Q_17", base, _with(blob, 11, 17)), ("W_4096", base, _with(blob, 1, 4096)),
                ("wrong_magic", base, _with(blob, 0, int(blob[0]) ^ 1))]
    out.append(("n_slots_0", "one_slot", _with(one, 9, 0)))
    out.append(("const_p", "plain", _with(plain, 12 + 2, P)))
    out.append(("n_chal_1_no_stage2", "plain", _with(plain, 5, 1)))
    nc = int(plain[6])
    grown = np.concatenate([plain[:12 + nc], np.zeros((1 << 16) - nc, dtype=np.uint64), plain[12 + nc:]])
    out.append(("n_const_65536", "plain", _with(grown, 6, 1 << 16)))
    s2 = 12 + int(perm[6]) + int(perm[7])
    out.append(("stage2_kind_3", "perm", _with(perm, s2, 3)))
    out.append(("stage2_column_W", "perm", _with(perm, s2 + 1, int(perm[1]))))
    return bases, out


def call_readers(bases, base, blob):
    """{reader: accepted}, and the words of zp_program_eval_ext where it accepted"""
    from eigen_zeth_amd import native
    good, trace, pubs, logn = bases[base]
    n_pub, n_chal, width = int(blob[4]), int(blob[5]), int(good[1]) + int(good[2])
    assert n_pub == len(pubs) and n_chal <= 3
    pubchal = list(pubs) + WC.EXPLICIT_CHALLENGE[:n_chal]
    zeta = [int(v) for v in O.random_field((3,), 4200)]
    ev_z, ev_zw = O.random_field((width, 3), 4201), O.random_field((width, 3), 4202)
    got, words = {}, None
    try:
        words = native.program_eval_ext(blob, pubchal, logn, ROOT32, zeta, ev_z, ev_zw)
        got["eval_ext"] = True
    except ValueError:
        got["eval_ext"] = False
    try:
        native.program_fixed_eval_ext(blob, pubchal, logn, ROOT32, zeta)
        got["fixed_eval_ext"] = True
    except ValueError:
        got["fixed_eval_ext"] = False
    try:
        native.program_fixed_eval_ext_batch(blob, [pubchal, pubchal], logn, ROOT32, [zeta, [5, 6, 7]])
        got["fixed_eval_ext_batch"] = True
    except ValueError:
        got["fixed_eval_ext_batch"] = False
    try:
        native.check_witness_host(blob, trace, pubs, logn, WC.EXPLICIT_CHALLENGE if int(blob[10]) else None, threads=1)
        got["check_witness"] = True
    except native.ZpError as e:
        assert e.code == -1
        got["check_witness"] = False
    prog = np.ascontiguousarray(blob)
    got["fixed_columns_words"] = int(native.load_library().zp_fixed_columns_words(prog.ctypes.data, prog.size, logn, 1)) != 0
    return got, words, (pubchal, logn, zeta, ev_z, ev_zw)


def oracle_words(blob, pubchal, logn, zeta, ev_z, ev_zw):
    """Program.evaluate_ext at zeta, or None where the checker's reader refuses the blob"""
    try:
        prog = Program(blob)
    except BadProgram:
        return None
    first, last = selectors_at(zeta, logn)
    pubs = pubchal[:int(blob[4])]
    fixed = [first, last] + [prog.fixed_eval_ext(k, pubs, zeta, logn, ROOT32) for k in range(len(prog.fixed_cols))]
    rows = lambda ev: [[int(v) for v in e] for e in ev]
    return prog.evaluate_ext(rows(ev_z), rows(ev_zw), fixed, pubchal, [(zeta[0] - w_last(logn)) % P, zeta[1], zeta[2]])


# accepted readers per (variant, base), in the order of READERS: e = eval_ext, f = fixed_eval_ext, b = its batch form, w = check_witness, c = fixed_columns_words
EXPECT = {
    ("good", "plain"): "efbwc", ("good", "perm"): "efbwc", ("good", "one_slot"): "efbwc",
    ("n_slots_0", "plain"): "fbc", ("n_slots_0", "perm"): "fbc",      # the code names slots above 0: zp_program_eval_ext refuses the operands, not the count
    ("n_slots_0", "one_slot"): "efbc",                                 # ... and reads the count as one slot
    ("n_slots_33", "plain"): "efbc", ("n_slots_33", "perm"): "efbc",
    ("n_slots_65537", "plain"): "c", ("n_slots_65537", "perm"): "c",
    ("Q_0", "plain"): "efbc", ("Q_0", "perm"): "efbc", ("Q_17", "plain"): "efbc", ("Q_17", "perm"): "efbc",
    ("W_4096", "plain"): "c", ("W_4096", "perm"): "c",
    ("wrong_magic", "plain"): "c", ("wrong_magic", "perm"): "c",
    ("const_p", "plain"): "efbc",
    ("n_chal_1_no_stage2", "plain"): "efbc",
    ("n_const_65536", "plain"): "efbc",
    ("stage2_kind_3", "perm"): "efbc", ("stage2_column_W", "perm"): "efbc",
}


def test_every_reader_takes_the_blobs_it_took():
    bases, vs = variants()
    seen, compared = {}, 0
    for name, base, blob in vs:
        got, words, args = call_readers(bases, base, blob)
        seen[(name, base)] = "".join(letter for letter, reader in zip("efbwc", READERS) if got[reader])
        if got["eval_ext"]:
            want = oracle_words(blob, *args)
            if want is not None:
                assert words.tolist() == want, (name, base)
                compared += 1
    assert seen == EXPECT
    assert compared >= 5
    # the differences the table exists for: each pair of readers is separated by some variant
    columns = {r: tuple(letter in seen[k] for k in sorted(seen)) for letter, r in zip("efbwc", READERS)}
    assert len({columns[r] for r in ("eval_ext", "fixed_eval_ext", "check_witness", "fixed_columns_words")}) == 4
    assert columns["fixed_eval_ext"] == columns["fixed_eval_ext_batch"]
