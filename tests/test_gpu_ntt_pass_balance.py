"""The NTT passes after the integer work was moved between them, word for word against the CPU oracle.

What changed in csrc/ntt.hip and what each case below runs:
  * plans of three passes or more: the pass before the last is plain and the LAST pass multiplies its loaded rows by that pass's
    inter-pass twiddle, from a table made once per plan (NttPlan::d_itab, [k][row], 1/N of an inverse plan folded in) --
    2^19 ([7,6,6]: radix-64 last pass, 32-column tiles, the smallest three-pass plan), 2^20 / 2^22 (mixed digits), 2^24 x 2
    ([8,8,8]: the kernels of the benchmark).  Forward: MODE 0 with the table; inverse: MODE 0 with the table and no output product
    at all.  The inverse side of an unfused extension (MODE 2: 1/N and coset powers on the outputs) takes no such table: the
    pass in front of it keeps its output-side one, from the same plan that runs zp_intt with the table.
    The plan says which path it takes ("last_pass_input_table" of zp_ntt_plan_json, false once the table failed to allocate);
    every case asserts it AFTER its transform ran, so no case can pass on the other path.
  * plans of two passes (2^13 the smallest, 2^18 the largest): the first pass feeds the last one directly, no input-side table;
    the inverse last pass writes its 1/N table once per workgroup instead of once per tile.
  * a zero-padded input exists only for a first pass (zp_lde without the seam kernel); the forward transforms of 2^19 and 2^20
    rows behind it are three-pass plans that end in an input-side table.
  * the seam kernel's built-in last pass takes no input-side table, so the pass in front of it keeps its output-side one
    (2^21: seam-role plans (7,6,8) + (8,7,7); 2^16: the default two-pass plans), with and without a coefficient store.
  * ntt_tw1 = 0: the per-lane chain form of the first pass in front of the same later passes.
  * a chunk seam: three columns run as 2 + 1, the table of the plan shared by both launches.
No A/B knob was left in the library, so there is no pair of settings to compare.

Inputs: O.random_field by seed with 0, P-1, 1 and 2^32 in front.  From 2^19 rows on the inverse transform is checked as
iNTT(O.ntt(x)) == x (one oracle transform per case)."""
import contextlib
import functools

import numpy as np
import pytest

from eigen_zeth_amd import native
from oracle import oracle as O

pytestmark = pytest.mark.gpu
P = O.P


@pytest.fixture(scope="module")
def p():
    pr = native.Prover(0)
    pr.set_profiling(True)
    yield pr
    pr.close()


@contextlib.contextmanager
def tuned(p, **knobs):
    """knobs of this module's own context, put back to the defaults of csrc/ctx.hpp afterwards"""
    defaults = {"ntt_chunk_log": 0, "lde_seam": 1, "ntt_tw1": 26}
    try:
        for k, v in knobs.items():
            p.set_tuning(k, v)
        yield
    finally:
        for k in knobs:
            p.set_tuning(k, defaults[k])


class Case:
    def __init__(self, logn, W):
        self.logn, self.W = logn, W
        self.x = O.random_field((W, 1 << logn), 11000 + 64 * logn + W)
        self.x[0, :4] = np.array([0, P - 1, 1, 2 ** 32], dtype=np.uint64)

    @functools.cached_property
    def fwd(self):
        return O.ntt(self.x)

    @functools.cached_property
    def inv(self):
        return O.intt(self.x)

    @functools.cached_property
    def ext(self):
        return O.lde(self.x, 1)

    @functools.cached_property
    def coef(self):
        return O.coset_scaled_coefficients(self.x)


@functools.lru_cache(maxsize=2)
def case(logn, W):
    return Case(logn, W)


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d words differ, first at (column, row) %s" % (what, len(bad), got.size, tuple(bad[0])))


def digits(p, logn):
    return [q["radix_log"] for q in p.ntt_plan(logn)["passes"]]


def drain(p):
    return [r for r, _ in p.pass_timings()]


def run_ntt(p, c, inverse, inplace, launches=1):
    """one zp_ntt / zp_intt call on c's columns; the launch sequence must be the plan's, `launches` times (column chunks)"""
    logn, W = c.logn, c.W
    if inverse:
        src, want = (c.x, c.inv) if logn <= 18 else (c.fwd, c.x)
    else:
        src, want = c.x, c.fwd
    what = "%s 2^%d x %d %s" % ("inverse" if inverse else "forward", logn, W, "in place" if inplace else "out of place")
    d_in = p.upload(src)
    d_out = d_in if inplace else p.alloc(W << logn)
    drain(p)
    (p.intt if inverse else p.ntt)(d_in, d_out, logn, W)
    d = digits(p, logn)
    assert drain(p) == ([-d[0]] + d[1:]) * launches, what + ": launches"
    assert p.ntt_plan(logn)["last_pass_input_table"] == (len(d) >= 3), what + ": input-side table of the last pass"
    same(p.download(d_out, src.shape), want, what)
    if not inplace:
        same(p.download(d_in, src.shape), src, what + ": input preserved")
        d_out.free()
    d_in.free()


def run_lde(p, c, coef, fused):
    logn, W = c.logn, c.W
    what = "extension 2^%d x %d by 2%s, %s" % (logn, W, " + coefficients" if coef else "", "seam kernel" if fused else "two transforms")
    d_in = p.upload(c.x)
    d_out = p.alloc(W << (logn + 1))
    d_coef = p.alloc(W << logn) if coef else None
    drain(p)
    p.lde(d_in, d_out, logn, 1, W, d_coef=d_coef)
    seq = drain(p)
    assert (88 in seq) == fused, what + ": route %s" % seq
    if not fused:      # a full inverse transform, then a full zero-padded forward one
        di, df = digits(p, logn), digits(p, logn + 1)
        assert seq == [-di[0]] + di[1:] + [-df[0]] + df[1:], what + ": launches %s" % seq
    assert p.ntt_plan(logn + 1)["last_pass_input_table"] == (len(digits(p, logn + 1)) >= 3), what + ": input-side table of the forward side"
    same(p.download(d_out, (W, 2 << logn)), c.ext, what)
    if coef:
        same(p.download(d_coef, c.x.shape), c.coef, what + ": coefficient store")
        d_coef.free()
    same(p.download(d_in, c.x.shape), c.x, what + ": input preserved")
    d_in.free()
    d_out.free()


SIZES = [(13, 3, [7, 6]), (18, 3, [9, 9]), (19, 3, [7, 6, 6]), (20, 3, [7, 7, 6]), (22, 3, [8, 7, 7]), (24, 2, [8, 8, 8])]


@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("logn,W,plan", SIZES, ids=[str(s[0]) for s in SIZES])
def test_transform(p, logn, W, plan, inverse, inplace):
    assert digits(p, logn) == plan
    run_ntt(p, case(logn, W), inverse, inplace)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_chunk_seam(p, inverse):
    """ntt_chunk_log = 21 at 2^20 rows: two columns per launch, so three columns run as 2 + 1"""
    with tuned(p, ntt_chunk_log=21):
        run_ntt(p, case(20, 3), inverse, inplace=False, launches=2)
        run_ntt(p, case(20, 3), inverse, inplace=True, launches=2)


@pytest.mark.parametrize("logn,fwd_plan", [(18, [7, 6, 6]), (19, [7, 7, 6])], ids=["to19", "to20"])
def test_zero_padded_input(p, logn, fwd_plan):
    """the zero-padded forward transforms of 2^19 and 2^20 rows (the second half of every input column reads as zero), behind an
    inverse transform whose last pass multiplies by 1/N and the coset powers"""
    with tuned(p, lde_seam=0):
        assert digits(p, logn + 1) == fwd_plan
        run_lde(p, case(logn, 3), coef=False, fused=False)


@pytest.mark.parametrize("coef", [False, True], ids=["nocoef", "coef"])
@pytest.mark.parametrize("logn,inv_plan,fwd_plan", [(16, [8, 8], [8, 9]), (21, [7, 6, 8], [8, 7, 7])], ids=["16", "21"])
def test_lde_seam(p, logn, inv_plan, fwd_plan, coef):
    """the fused extension: 2^16 the smallest size with a seam kernel, 2^21 the smallest on seam-role plans"""
    with tuned(p, lde_seam=2):
        lde = p.ntt_plan(logn)["lde"]
        assert lde["seam_fused"] and lde["inverse_radix_logs"] == inv_plan and lde["forward_radix_logs"] == fwd_plan, lde
        run_lde(p, case(logn, 3), coef, fused=True)


@pytest.mark.parametrize("coef", [False, True], ids=["nocoef", "coef"])
def test_lde_unfused_three_pass_inverse(p, coef):
    """lde_seam = 0 at 2^21: the inverse plan (7,7,7) ends in a MODE 2 pass (1/N and coset powers on the outputs, the pass before it
    with its output-side table); the zero-padded forward plan (8,7,7) behind it ends in an input-side table"""
    with tuned(p, lde_seam=0):
        assert digits(p, 21) == [7, 7, 7] and digits(p, 22) == [8, 7, 7]
        run_lde(p, case(21, 3), coef, fused=False)


@pytest.mark.parametrize("logn", [18, 20])
def test_first_pass_chain(p, logn):
    """ntt_tw1 = 0: the first pass on per-lane chains gives the same words into the same later passes"""
    with tuned(p, ntt_tw1=0):
        assert not p.ntt_plan(logn)["first_pass_table"]
        run_ntt(p, case(logn, 3), inverse=False, inplace=False)
        run_ntt(p, case(logn, 3), inverse=True, inplace=True)
