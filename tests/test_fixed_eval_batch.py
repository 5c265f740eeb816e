"""zp_program_fixed_eval_ext_batch: the fixed columns of a program at many points, each with its own public inputs.
Programs are written by hand from the documented blob layout (include/zeth_prover.h, "constraint program"): no prover is needed.  The expected
words come from the checker's own reader (oracle/air_program.py: fixed_eval_ext; the two selectors from tests/test_program_cases.py).  The host half
(ctx = NULL) runs anywhere; the device half asks for the host call's words exactly, on both sides of the knob "fixed_eval_dev_min".
Sizes: a workgroup of csrc/fixed_eval.hip takes up to 1024 entries of a column on 256 lanes, so besides the lengths around one wave (63, 64, 65) and
one workgroup (257) there are columns of 1023, 1024, 1025 and 2500 entries -- a column cut into one, two and three segments.  (A column of 65 entries
needs a period of 128 rows, so it sits in the 2^9-row program beside the one of 257, not in a 2^6-row one.)"""
import numpy as np
import pytest

from oracle import naive as NV
from oracle import oracle as O
from oracle.air_program import MAGIC, Program
from test_program_cases import selectors_at

P = O.P
ROOT32 = O.ROOT32_DEFAULT
PUB = 1 << 63


def blob_of(cols, n_pub):
    """a program of one trace column and one constraint (OUT column 0) whose sparse fixed columns are `cols`: [(lp, [(pos, is_pub, value or index)])]"""
    w = [MAGIC, 1, 0, 2 + len(cols), n_pub, 0, 0, 1, 1, 0, 0, 1, 4 | (1 << 24)]
    for lp, ent in cols:
        w.append(lp | (len(ent) << 8))
        for pos, is_pub, v in ent:
            w += [pos | (PUB if is_pub else 0), v]
    return np.array(w, dtype=np.uint64)


def column(lp, n, seed, pubs=()):
    """n entries at distinct positions of a period of 2^lp rows, the last position among them; `pubs`: (entry number, public index) pairs"""
    rng = np.random.default_rng(seed)
    pos = sorted(set([(1 << lp) - 1] + [int(v) for v in rng.permutation((1 << lp) - 1)[:n - 1]])) if n else []
    assert len(pos) == n
    vals = [int(v) for v in O.random_field((n + 1,), seed + 1)]
    ent = [(p, False, vals[i] or 1) for i, p in enumerate(pos)]
    for i, k in pubs:
        ent[i] = (ent[i][0], True, k)
    return (lp, ent)


def programs():
    """name -> (blob, logn, n_pub)"""
    small = [column(6, 0, 100), column(0, 1, 110), column(3, 1, 120), column(6, 63, 130), column(6, 64, 140, pubs=((0, 0), (5, 1), (63, 2))),
             (2, [(3, False, P - 1), (0, True, 1)]), (5, [(31, True, 2), (7, False, 0), (9, False, 5)])]
    mid = [column(7, 65, 200), column(9, 257, 210, pubs=((256, 0),)), column(0, 0, 220)]
    big = [column(10, 1023, 300), column(10, 1024, 310), column(11, 1025, 320, pubs=((1024, 0),)), column(12, 2500, 330), column(1, 2, 340)]
    return {"none": (blob_of([], 2), 6, 2), "small": (blob_of(small, 3), 6, 3), "mid": (blob_of(mid, 1), 9, 1), "big": (blob_of(big, 1), 12, 1)}


def points(name, n_points, n_pub, logn):
    """(public inputs [n_points][n_pub], zeta [n_points][3]): random points; point 0 of a call of more than one lies in the base field, and the
    public input 1 of every odd point is 0"""
    seed = 5000 + 31 * n_points + sum(map(ord, name))
    zeta = [[int(v) for v in row] for row in O.random_field((n_points, 3), seed)]
    pubs = [[int(v) for v in row] for row in O.random_field((n_points, max(n_pub, 1)), seed + 1)]
    pubs = [row[:n_pub] for row in pubs]
    if n_points > 1:
        zeta[0] = [zeta[0][0], 0, 0]
    for i in range(1, n_points, 2):
        if n_pub > 1:
            pubs[i][1] = 0
    return pubs, zeta


def expected(blob, pubs, zeta, logn):
    prog = Program(blob)
    out = []
    for pb, z in zip(pubs, zeta):
        first, last = selectors_at(z, logn)
        out.append([first, last] + [prog.fixed_eval_ext(k, pb, z, logn, ROOT32) for k in range(len(prog.fixed_cols))])
    return out


CASES = [("none", 2), ("small", 1), ("small", 2), ("small", 67), ("mid", 2), ("big", 2)]
_memo = {}


def case(name, n_points):
    """(blob, logn, pubs, zeta, the checker's words), made once and left unchanged"""
    key = (name, n_points)
    if key not in _memo:
        blob, logn, n_pub = programs()[name]
        pubs, zeta = points(name, n_points, n_pub, logn)
        _memo[key] = (blob, logn, pubs, zeta, expected(blob, pubs, zeta, logn))
    return _memo[key]


def on_domain_case():
    """the "small" program at five points: point 2 is w_64^5, position 5 of the period of the column that fills all 64 rows (zeta^(N/p) = w_p^pos with
    p = N); point 3 is the first row itself, where the selector has its pole.  The three other points are random and must come out as if alone."""
    blob, logn, n_pub = programs()["small"]
    pubs, zeta = points("domain", 5, n_pub, logn)
    w = NV.root(logn, ROOT32)
    zeta[2] = [pow(w, 5, P), 0, 0]
    zeta[3] = [1, 0, 0]
    return blob, logn, pubs, zeta, [False, False, True, True, False]


def zero_public_case():
    """one column of period 8 with a public entry at position 5 and a constant one at 2, 2^6 rows: zeta = w_64^5 meets the public entry.  Where that
    public input is 0 the entry is no term of the sum, so the column has no pole there: points 0 and 1 are the same zeta with the public input 0 and 7;
    only point 1 is on the column's domain.  (zeta is a trace row, so Z_H(zeta) = 0 and every value of point 0 is 0 -- but not flagged.)"""
    blob = blob_of([(3, [(5, True, 0), (2, False, 9)])], 1)
    w = NV.root(6, ROOT32)
    z = [pow(w, 5, P), 0, 0]
    return blob, 6, [[0], [7], [3]], [z, z, [11, 12, 13]], [False, True, False]


def check_against_checker(got, flags, want):
    assert not flags.any()
    assert got.tolist() == want


@pytest.mark.parametrize("name,n_points", CASES)
def test_host_batch_matches_the_checker(name, n_points):
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, want = case(name, n_points)
    got, flags = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta)
    check_against_checker(got, flags, want)
    # ... and the single-point call, point by point
    for i in range(n_points):
        assert native.program_fixed_eval_ext(blob, pubs[i], logn, ROOT32, zeta[i]).tolist() == got[i].tolist()


@pytest.mark.parametrize("make", [on_domain_case, zero_public_case])
def test_host_batch_flags_a_point_on_a_domain_and_no_other(make):
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, want_flags = make()
    got, flags = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta)
    assert flags.tolist() == want_flags
    for i, f in enumerate(want_flags):
        if f:
            assert not got[i].any()
            with pytest.raises(ValueError):                     # the single-point call refuses what the batch flags
                native.program_fixed_eval_ext(blob, pubs[i], logn, ROOT32, zeta[i])
        else:
            assert got[i].tolist() == expected(blob, [pubs[i]], [zeta[i]], logn)[0]


def test_host_batch_refusals_are_the_single_calls():
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, _ = case("small", 2)
    native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta)
    with pytest.raises(ValueError):                             # truncated blob
        native.program_fixed_eval_ext_batch(blob[:-1], pubs, logn, ROOT32, zeta)
    with pytest.raises(ValueError):                             # a zeta word >= p in the SECOND point
        native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, [zeta[0], [P, 0, 0]])
    with pytest.raises(ValueError):                             # a public input >= p in the second point
        native.program_fixed_eval_ext_batch(blob, [pubs[0], [P] + pubs[1][1:]], logn, ROOT32, zeta)
    with pytest.raises(ValueError):                             # another count of public inputs than the program's
        native.program_fixed_eval_ext_batch(blob, [r[:-1] for r in pubs], logn, ROOT32, zeta)
    with pytest.raises(ValueError):                             # a column longer than the trace
        native.program_fixed_eval_ext_batch(blob, pubs, 5, ROOT32, zeta)
    bad = blob.copy()
    bad[3] += 1                                                 # n_fixed that is not the table's
    with pytest.raises(ValueError):
        native.program_fixed_eval_ext_batch(bad, pubs, logn, ROOT32, zeta)
    # the caller's n_fixed against the program's, and null pointers: straight through the C ABI
    import ctypes as C
    lib = native.load_library()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    pc, z = np.array(pubs, dtype=np.uint64).reshape(-1), np.array(zeta, dtype=np.uint64).reshape(-1)
    out, fl = np.zeros((2, int(blob[3]) + 1, 3), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    flp = fl.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.zp_program_fixed_eval_ext_batch(None, p(blob), blob.size, p(pc), 3, logn, ROOT32, p(z), 2, p(out), int(blob[3]), flp, 0) == 0
    assert lib.zp_program_fixed_eval_ext_batch(None, p(blob), blob.size, p(pc), 3, logn, ROOT32, p(z), 2, p(out), int(blob[3]) + 1, flp, 0) == -1
    assert lib.zp_program_fixed_eval_ext_batch(None, None, blob.size, p(pc), 3, logn, ROOT32, p(z), 2, p(out), int(blob[3]), flp, 0) == -1
    assert lib.zp_program_fixed_eval_ext_batch(None, p(blob), blob.size, p(pc), 3, logn, ROOT32, None, 2, p(out), int(blob[3]), flp, 0) == -1
    assert lib.zp_program_fixed_eval_ext_batch(None, p(blob), blob.size, p(pc), 3, logn, ROOT32, p(z), 2, p(out), int(blob[3]), None, 0) == -1


# ---- the device half: the host call's words exactly, whichever side of the knob

@pytest.fixture(params=[0, 2**31 - 1], ids=["device", "host"])
def dev_min(prover, request):
    prover.set_tuning("fixed_eval_dev_min", request.param)
    yield request.param
    prover.set_tuning("fixed_eval_dev_min", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_points", CASES)
def test_device_batch_gives_the_host_words(prover, dev_min, name, n_points):
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, want = case(name, n_points)
    host, host_flags = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta)
    got, flags = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta, prover=prover)
    assert flags.tolist() == host_flags.tolist() and (got == host).all()
    check_against_checker(got, flags, want)
    again, _ = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta, prover=prover)      # the tables now come from the ctx
    assert (again == host).all()


@pytest.mark.gpu
@pytest.mark.parametrize("make", [on_domain_case, zero_public_case])
def test_device_batch_flags_the_same_points(prover, dev_min, make):
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, want_flags = make()
    host, _ = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta)
    got, flags = native.program_fixed_eval_ext_batch(blob, pubs, logn, ROOT32, zeta, prover=prover)
    assert flags.tolist() == want_flags and (got == host).all()


@pytest.mark.gpu
def test_device_batch_refuses_what_the_host_refuses(prover, dev_min):
    from eigen_zeth_amd import native
    blob, logn, pubs, zeta, _ = case("small", 2)
    for args in ((blob[:-1], pubs, logn, zeta), (blob, pubs, logn, [zeta[0], [P, 0, 0]]), (blob, [pubs[0], [P] + pubs[1][1:]], logn, zeta), (blob, pubs, 5, zeta)):
        with pytest.raises(ValueError):
            native.program_fixed_eval_ext_batch(args[0], args[1], args[2], ROOT32, args[3], prover=prover)


@pytest.mark.gpu
def test_the_knob_is_known_and_a_program_evicted_from_the_ctx_is_rebuilt(prover):
    """five programs in turn through a ctx that keeps the tables of four: the first is made again, same words"""
    from eigen_zeth_amd import native
    prover.set_tuning("fixed_eval_dev_min", 0)
    try:
        blobs = [blob_of([column(4, 9, 900 + k)], 0) for k in range(5)]
        zeta = [[3, 4, 5], [6, 0, 0]]
        first = native.program_fixed_eval_ext_batch(blobs[0], [[], []], 6, ROOT32, zeta, prover=prover)[0]
        for b in blobs[1:]:
            got = native.program_fixed_eval_ext_batch(b, [[], []], 6, ROOT32, zeta, prover=prover)[0]
            assert (got == native.program_fixed_eval_ext_batch(b, [[], []], 6, ROOT32, zeta)[0]).all()
        assert (native.program_fixed_eval_ext_batch(blobs[0], [[], []], 6, ROOT32, zeta, prover=prover)[0] == first).all()
        # the same program on another trace length is another table
        assert (native.program_fixed_eval_ext_batch(blobs[0], [[], []], 7, ROOT32, zeta, prover=prover)[0] ==
                native.program_fixed_eval_ext_batch(blobs[0], [[], []], 7, ROOT32, zeta)[0]).all()
    finally:
        prover.set_tuning("fixed_eval_dev_min", -1)
