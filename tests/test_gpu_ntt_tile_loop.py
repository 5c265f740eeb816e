"""The tile loop of ntt_pass2_kernel (csrc/ntt.hip) at every trip count and in every kind of instantiation, word for word
against the CPU oracle.

The loop runs two tiles a trip with its two register sets in swapped roles, so a workgroup's `tiles_per_wg` tiles are walked
by the first body alone (1), by both bodies once (2) and by more than one trip (4); the limb form keeps one tile a trip.
Which tables a pass has is a template argument (TAB_NONE / TAB_FIXED / TAB_TILE / TAB_IN), chosen by launch_pass2 from what
run_one_pass asks for.  The cases:

  2^16 x 256   plan [8, 8]: a first pass and a TAB_NONE (forward) / TAB_FIXED (inverse, 1/N) last pass of shape (4,4,0,4), 16
               tiles a pass.  256 columns keep ntt_tpw = 2 and 4 alive through the rule of launch_pass2; 3 must run as 1.  At
               4 the first pass's grid is 4 workgroups a column, no multiple of the 8 XCDs: it runs the per-lane chain.
  2^24 x 2     the only size here whose plan is [8, 8, 8]: the table first pass, the TAB_NONE middle pass and the last pass
               with the input-side table (TAB_IN) -- the instantiations of the benchmark.
  2^20 x 16    extension by 2 in two launches per side: the zero-padded first pass and the last pass that multiplies by coset
               powers (MODE 2), with and without the coefficient store; the passes between them carry TAB_TILE.
  2^19 x 32    forward on the limb form.

Every run reads the launch sequence back (pass_timings) and compares it with the plan.  The module owns its context; each
knob is put back in `finally`.  Oracle results are computed once per size."""
import contextlib
import functools
import os
import re

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


def _ctx_default(key):
    field = {"ntt_tpw": "tpw"}.get(key, key)
    with open(os.path.join(os.path.dirname(native.__file__), "csrc", "ctx.hpp")) as f:
        return int(dict(re.findall(r"\btune_(\w+) = (-?\d+)", f.read()))[field])


@contextlib.contextmanager
def tuned(p, **knobs):
    try:
        for k, v in knobs.items():
            p.set_tuning(k, v)
        yield
    finally:
        for k in knobs:
            p.set_tuning(k, _ctx_default(k))


class Case:
    def __init__(self, logn, W):
        self.logn, self.W = logn, W
        self.x = O.random_field((W, 1 << logn), 12000 + 64 * logn + W)
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
        raise AssertionError("%s: %d of %d elements differ, first at (column, row) %s" % (what, len(bad), got.size, tuple(bad[0])))


def digits(p, logn):
    return [q["radix_log"] for q in p.ntt_plan(logn)["passes"]]


def launches(d):
    return [-d[0]] + list(d[1:])


def drain(p):
    return [r for r, _ in p.pass_timings()]


def surviving_tpw(tpw, tiles, W, cus):
    """the loop of launch_pass2"""
    while tpw > 1 and (tiles % tpw != 0 or tiles // tpw * W < 4 * cus):
        tpw >>= 1
    return tpw


def run_forward(p, c, what):
    d_in, d_out = p.upload(c.x), p.alloc(c.W << c.logn)
    drain(p)
    p.ntt(d_in, d_out, c.logn, c.W)
    assert drain(p) == launches(digits(p, c.logn)), what + ": launches"
    same(p.download(d_out, c.x.shape), c.fwd, what + " forward")
    d_in.free()
    d_out.free()


def run_inverse(p, c, what):
    """up to 2^18 rows iNTT(x) against O.intt(x); above, iNTT(O.ntt(x)) against x (one oracle transform less)"""
    src, want = (c.x, c.inv) if c.logn <= 18 else (c.fwd, c.x)
    d = p.upload(src)
    drain(p)
    p.intt(d, d, c.logn, c.W)
    assert drain(p) == launches(digits(p, c.logn)), what + ": launches"
    same(p.download(d, c.x.shape), want, what + " inverse")
    d.free()


@pytest.mark.parametrize("tpw", [1, 2, 4, 3])
def test_two_pass_every_trip_count(p, tpw):
    """2^16 rows x 256 columns, plan [8, 8], 16 tiles a pass"""
    cus = p.device_info()["cus"]
    want = {1: 1, 2: 2, 4: 4, 3: 1}[tpw]
    c = case(16, 256)
    with tuned(p, ntt_tpw=tpw):
        plan = p.ntt_plan(16)
        assert digits(p, 16) == [8, 8] and all(q["tile"] == 16 and q["rounds"] == [4, 4, 0] for q in plan["passes"]), plan
        tiles = (1 << 16) // 256 // 16
        assert tiles == 16 and surviving_tpw(tpw, tiles, c.W, cus) == want, (tpw, cus)
        # the table form of the first pass needs a grid of a multiple of 8 workgroups a column: gone at 4 tiles a workgroup
        assert plan["first_pass_table"] and ((tiles // want) % 8 == 0) == (want <= 2)
        run_forward(p, c, "2^16 x 256 ntt_tpw=%d" % tpw)
        run_inverse(p, c, "2^16 x 256 ntt_tpw=%d" % tpw)


@pytest.mark.parametrize("tpw", [1, 2, 4])
def test_three_pass_bench_instantiations(p, tpw):
    """2^24 rows x 2 columns, plan [8, 8, 8]: table first pass, plain middle pass, last pass with the input-side table"""
    cus = p.device_info()["cus"]
    c = case(24, 2)
    with tuned(p, ntt_tpw=tpw):
        plan = p.ntt_plan(24)
        assert digits(p, 24) == [8, 8, 8] and plan["first_pass_table"] and plan["last_pass_input_table"], plan
        tiles = (1 << 24) // 256 // 16
        assert surviving_tpw(tpw, tiles, c.W, cus) == tpw and (tiles // tpw) % 8 == 0, (tpw, cus)
        run_forward(p, c, "2^24 x 2 ntt_tpw=%d" % tpw)
        run_inverse(p, c, "2^24 x 2 ntt_tpw=%d" % tpw)


@pytest.mark.parametrize("coef", [False, True], ids=["plain", "coef"])
@pytest.mark.parametrize("tpw", [1, 4])
def test_extension_two_launches(p, tpw, coef):
    """2^20 rows x 16 columns by 2, each side a transform of its own: MODE 2 last pass of the inverse side, zero-padded first
    pass of the forward side"""
    cus = p.device_info()["cus"]
    c = case(20, 16)
    what = "extension 2^20 x 16 ntt_tpw=%d%s" % (tpw, " + coefficients" if coef else "")
    with tuned(p, ntt_tpw=tpw, lde_seam=0):
        assert not p.ntt_plan(20)["lde"]["seam_fused"]
        for logn in (20, 21):
            for q in p.ntt_plan(logn)["passes"]:
                assert surviving_tpw(tpw, ((1 << logn) >> q["radix_log"]) // q["tile"], c.W, cus) == tpw, (logn, q, cus)
        d_in, d_out = p.upload(c.x), p.alloc(c.W << 21)
        d_coef = p.alloc(c.W << 20) if coef else None
        drain(p)
        p.lde(d_in, d_out, 20, 1, c.W, d_coef=d_coef)
        assert drain(p) == launches(digits(p, 20)) + launches(digits(p, 21)), what + ": launches"
        same(p.download(d_out, (c.W, 1 << 21)), c.ext, what)
        if coef:
            same(p.download(d_coef, c.x.shape), c.coef, what + ": coefficient store")
            d_coef.free()
        same(p.download(d_in, c.x.shape), c.x, what + ": input preserved")
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("tpw", [1, 2])
def test_limb_form(p, tpw):
    """2^19 rows x 32 columns forward on limbs: every pass of [7, 6, 6] is at most radix 256 and the first has its table"""
    cus = p.device_info()["cus"]
    c = case(19, 32)
    with tuned(p, ntt_tpw=tpw, ntt_limb=1):
        plan = p.ntt_plan(19)
        assert digits(p, 19) == [7, 6, 6] and plan["first_pass_table"], plan
        for q in plan["passes"]:
            tiles = ((1 << 19) >> q["radix_log"]) // q["tile"]
            assert surviving_tpw(tpw, tiles, c.W, cus) == tpw and (tiles // tpw) % 8 == 0, (q, cus)
        run_forward(p, c, "limb 2^19 x 32 ntt_tpw=%d" % tpw)
