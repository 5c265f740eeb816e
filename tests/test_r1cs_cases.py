"""The seeded small circuits of tests/r1cs_cases.py, on the CPU: for every shape the library's host evaluator (zp_r1cs_eval) equals
Circuit.complete word for word, the checker's own reader of the blob (oracle/r1cs_blob.py) finds no violated row, and the blob has the wave
bounds and the domain the shape is meant to have -- so that the device tests (tests/test_gpu_r1cs_device.py) stand on circuits that are what
they claim to be.  Also the refusals the device tests compare: the host's code and *bad for each fault; and the key generator's scalars on the
two shapes in which gadget rows, explicit rows and arithmetic rows meet in one key."""
import numpy as np
import pytest

import r1cs_cases as RC
from eigen_zeth_amd import native
from oracle import r1cs_blob as RB


def _waves(blob):
    """the wave bounds of a blob, read by offsets (csr sizes from the blob itself)"""
    d = [int(v) for v in blob]
    t, tc, n_inst, n_waves = d[4], d[6], d[7], d[10]
    at = 16 + tc
    for _ in range(3):
        nnz = d[at + tc]
        at += tc + 1 + 5 * nnz
    at += n_inst * (t + 2)
    return d[at:at + n_waves + 1]


@pytest.mark.parametrize("name", sorted(RC.SHAPES))
def test_host_evaluator_equals_the_reference_on_every_shape(name):
    cs = RC.case(name)
    assert _waves(cs.blob) == RC.WAVE_BOUNDS[name] and cs.logm == RC.LOGM[name] and cs.n_pub == RC.SHAPES[name][5]
    ref = cs.circuit.complete(cs.vals)
    wf, a, b, c = native.r1cs_eval(cs.blob, *cs.arrays())
    assert native.fr_ints(wf) == ref
    assert RB.first_violated(cs.blob, ref) == -1
    assert not a[cs.n_cons:].any() and not b[cs.n_cons:].any() and not c[cs.n_cons:].any()
    print("%s: %d wires, %d constraints, domain 2^%d" % (name, cs.n_wires, cs.n_cons, cs.logm))


def test_shapes_sit_on_the_seams_they_are_meant_for():
    s2, s3, s4 = RC.case("S2"), RC.case("S3"), RC.case("S4")
    n_extra = int(s3.blob[8])
    assert n_extra > 256 + 40 and len(s3.tags["defined"]) == 40 and len(s3.tags["arith_inputs"]) == 257
    # finding 1's shape: an explicit definition and a gadget input inside an arithmetic instance's internal range
    T, _ = RC.arith_template()
    inside = lambda w: any(base <= w < base + T.n_int for _, base in s4.circuit.ariths[0][1])
    q, w = s4.tags["def_reads_arith"]
    assert inside(w) and s4.circuit.extras[q][3] is not None and w in s4.circuit.extras[q][1]
    i, w = s4.tags["gadget_reads_arith"]
    assert inside(w) and w in s4.circuit.instances[i][0] and s4.circuit.instances[i][2] == 0
    # the refusal tests' wires have the one reader their tag names
    c = s2.circuit
    readers = lambda w: ([("gadget", i) for i, it in enumerate(c.instances) if w in it[0]] +
                         [("row", q) for q, e in enumerate(c.extras) if any(w in M for M in e[:3])])
    assert readers(s2.tags["only_wave1"]) == [("gadget", 10)] and readers(s2.tags["only_plain"]) == [("row", s2.tags["plain_row"][0])]
    assert readers(s2.tags["only_mid_def"]) == [("row", s2.tags["mid_def"][0])] and readers(s2.tags["unread"]) == []
    assert ("gadget", 0) in readers(s2.tags["wave0_input"])
    assert s2.vals != RC.case("S2", 9).vals and (s2.blob == RC.case("S2", 9).blob).all()


def test_host_refusals_name_the_row_or_wire_at_fault():
    cs = RC.case("S2")
    t = cs.tags
    base = 12 * RC.TC
    first_arith = base + int(cs.blob[8])
    d_at = len(t["defined"]) // 2 - 1
    d_row = [q for q, e in enumerate(cs.circuit.extras) if e[3] == t["defined"][d_at]][0]
    want = {"unset: wave0_input": (-21, 0), "unset: only_wave1": (-21, 10 * RC.TC), "unset: only_plain": (-21, base + t["plain_row"][0]),
            "unset: only_mid_def": (-21, base + t["mid_def"][0]), "unset: arith_input": (-21, first_arith), "unset: unread": (-21, t["unread"]),
            "violated: a defined wire set off by one": (-20, base + d_row), "violated: a plain row": (-20, base + t["plain_row"][0]),
            "violated: a plain row, in the top limb only": (-20, base + t["plain_row"][0]),
            "violated: e3_inv of zero in the second arithmetic instance": (-20, first_arith + t["arith_rows"])}
    got = {k: RC.host_refusal(cs, v) for k, v in RC.faults(cs).items()}
    assert got == want


@pytest.mark.parametrize("name", ["S2", "S4"])
def test_key_scalars_match_the_definition_where_the_three_row_kinds_meet(name):
    """zp_r1cs_key_scalars against u_j = sum_i A[i][j] L_i(tau) (v, w alike) in Python integers over Circuit.rows(): gadget instances, explicit
    rows and arithmetic instances add into the same wires' scalars (S4: an arithmetic instance's internal wire read by a gadget and by a row)"""
    cs = RC.case(name)
    c, R = cs.circuit, RC.R
    tau, al, be, ga, de = 123456789, 5, 7, 11, 13
    u, v, l, h = native.r1cs_key_scalars(cs.blob, tau, al, be, ga, de)
    m, om = 1 << cs.logm, pow(5, (R - 1) >> cs.logm, R)
    zt = (pow(tau, m, R) - 1) % R
    rows = list(c.rows())
    assert len(rows) == cs.n_cons
    wp = [1]
    for _ in range(len(rows) - 1):
        wp.append(wp[-1] * om % R)
    scale = zt * pow(m, -1, R) % R
    den, pre, run = [(tau - x) % R for x in wp], [], 1                # 1 / (tau - w^i): one inversion for all of them
    for d in den:
        pre.append(run)
        run = run * d % R
    inv, L = pow(run, -1, R), [0] * len(rows)
    for i in range(len(rows) - 1, -1, -1):
        L[i] = scale * wp[i] % R * (inv * pre[i] % R) % R
        inv = inv * den[i] % R
    acc = [[0] * cs.n_wires for _ in range(3)]
    for Li, row in zip(L, rows):
        for a, M in zip(acc, row):
            for k, cf in M.items():
                a[k] = (a[k] + cf * Li) % R
    assert native.fr_ints(u) == acc[0] and native.fr_ints(v) == acc[1]
    dinv, ginv = pow(de, -1, R), pow(ga, -1, R)
    assert native.fr_ints(l) == [(be * acc[0][j] + al * acc[1][j] + acc[2][j]) * (ginv if j <= cs.n_pub else dinv) % R for j in range(cs.n_wires)]
    hi = native.fr_ints(h)
    assert len(hi) == m - 1 and hi[0] == zt * dinv % R and hi[m - 2] == pow(tau, m - 2, R) * zt * dinv % R
    e0 = 12 * RC.TC
    e1 = e0 + int(cs.blob[8])
    gadget, explicit, arith = (set(k for row in rows[a:b] for M in row for k in M) - {0} for a, b in ((0, e0), (e0, e1), (e1, cs.n_cons)))
    assert gadget & explicit and arith and (name != "S4" or (gadget & arith and explicit & arith))      # one wire's scalar takes terms of two row kinds
