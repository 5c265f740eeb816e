"""The LDS slot addresses of the NTT passes on the GPU, word for word against the CPU oracle.

csrc/ntt.hip computes a slot's LDS address in factors (csrc/ntt_geo.hpp: a lane part per round, the uniform bits of k_j, one XOR per
write; the table copy-out reads at the lane part XOR a constant and walks its table and destination rows by scalar adds).  The host
program of tests/test_ntt_slots.py proves the address identities; here every kernel form that takes them runs:

  * every pass shape reachable at the default knobs, as a first pass and as a later pass, at the smallest 2^13 .. 2^22 rows whose plan
    (prover.ntt_plan) has it there -- 3 columns, forward and inverse (the default root: j0inv 5 and 11), in place and out of place;
  * 2^24 rows x 2 forward: the three instantiations of the benchmark (table first pass, plain middle pass, last pass with the input-side
    table), at ntt_tpw = 1, the default and 4 (two tiles a trip once, twice);
  * 2^16 x 3 with ntt_logt = 5 (32-column tiles: the swizzle takes k_j in the last round too), ntt_tw1 = 0 (per-lane chain: keeps lpos in
    its exchange), ntt_limb = 1 (limb rounds keep lpos, the copy-out is shared);
  * the extension by 2 at 2^16 on both routes: lde_seam_kernel, and the zero-padded first pass behind a MODE 2 last pass.

The module owns its context; every knob is put back in `finally`.  Oracle results are computed once per size."""
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
_FIELD = {"ntt_logt": "logt", "ntt_tpw": "tpw"}


@pytest.fixture(scope="module")
def p():
    pr = native.Prover(0)
    pr.set_profiling(True)
    yield pr
    pr.close()


def _ctx_default(key):
    with open(os.path.join(os.path.dirname(native.__file__), "csrc", "ctx.hpp")) as f:
        return int(dict(re.findall(r"\btune_(\w+) = (-?\d+)", f.read()))[_FIELD.get(key, key)])


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
        self.x = O.random_field((W, 1 << logn), 13000 + 64 * logn + W)
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


@functools.lru_cache(maxsize=None)
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


def run_forward(p, c, inplace, what):
    d_in = p.upload(c.x)
    d_out = d_in if inplace else p.alloc(c.W << c.logn)
    drain(p)
    p.ntt(d_in, d_out, c.logn, c.W)
    assert drain(p) == launches(digits(p, c.logn)), what + ": launches"
    same(p.download(d_out, c.x.shape), c.fwd, "%s forward %s" % (what, "in place" if inplace else "out of place"))
    if not inplace:
        same(p.download(d_in, c.x.shape), c.x, what + " forward: input preserved")
        d_out.free()
    d_in.free()


def run_inverse(p, c, inplace, what):
    """iNTT(O.ntt(x)) against x: the forward oracle result is there already"""
    d_in = p.upload(c.fwd)
    d_out = d_in if inplace else p.alloc(c.W << c.logn)
    drain(p)
    p.intt(d_in, d_out, c.logn, c.W)
    assert drain(p) == launches(digits(p, c.logn)), what + ": launches"
    same(p.download(d_out, c.x.shape), c.x, "%s inverse %s" % (what, "in place" if inplace else "out of place"))
    if not inplace:
        d_out.free()
    d_in.free()


def run_all_four(p, c, what):
    for inplace in (False, True):
        run_forward(p, c, inplace, what)
        run_inverse(p, c, inplace, what)


def shape_of(q):
    return tuple(q["rounds"]) + (q["tile"],)


def default_shape_sizes(p):
    """{logn: [(shape, 'first' | 'later'), ..]}: for every shape a default plan of 2^13 .. 2^22 rows has, the smallest size that runs
    it as a first pass and the smallest that runs it as a later pass"""
    first, later = {}, {}
    for logn in range(13, 23):
        passes = p.ntt_plan(logn)["passes"]
        first.setdefault(shape_of(passes[0]), logn)
        for q in passes[1:]:
            later.setdefault(shape_of(q), logn)
    sizes = {}
    for role, found in (("first", first), ("later", later)):
        for s, logn in found.items():
            sizes.setdefault(logn, []).append((s, role))
    return sizes


def test_every_default_shape_first_and_later(p):
    """3 columns, forward and inverse, in place and out of place, at the sizes default_shape_sizes picks"""
    sizes = default_shape_sizes(p)
    seen = {s for v in sizes.values() for s, _ in v}
    # radix 64, 128, 256 on two rounds, radix 512 on three: what dispatch_pass is asked for below 2^23 rows at the default knobs; the
    # balanced plans bring each of them to both places by 2^18 rows (radix 64 is the first digit of no plan)
    assert seen == {(3, 3, 0, 32), (4, 3, 0, 32), (4, 4, 0, 16), (3, 3, 3, 16)}, sizes
    assert sum(len(v) for v in sizes.values()) == 7 and max(sizes) <= 18, sizes
    for logn, roles in sorted(sizes.items()):
        run_all_four(p, case(logn, 3), "2^%d x 3 %s" % (logn, roles))


@pytest.mark.parametrize("tpw", [None, 1, 4], ids=["default", "tpw1", "tpw4"])
def test_bench_instantiations(p, tpw):
    """2^24 rows x 2 columns forward, plan [8, 8, 8]: table first pass, plain middle pass, last pass with the input-side table"""
    c = case(24, 2)
    with tuned(p, **({} if tpw is None else {"ntt_tpw": tpw})):
        plan = p.ntt_plan(24)
        assert digits(p, 24) == [8, 8, 8] and plan["first_pass_table"] and plan["last_pass_input_table"], plan
        assert all(shape_of(q) == (4, 4, 0, 16) for q in plan["passes"]), plan
        run_forward(p, c, False, "2^24 x 2 ntt_tpw=%s" % tpw)


@pytest.mark.parametrize("knob,value", [("ntt_logt", 5), ("ntt_tw1", 0), ("ntt_limb", 1)])
def test_one_knob(p, knob, value):
    c = case(16, 3)
    with tuned(p, **{knob: value}):
        plan = p.ntt_plan(16)
        assert digits(p, 16) == [8, 8], plan
        assert [q["tile"] for q in plan["passes"]] == ([32, 32] if knob == "ntt_logt" else [16, 16]), plan
        assert plan["first_pass_table"] == (knob != "ntt_tw1"), plan
        run_forward(p, c, False, "2^16 x 3 %s=%d" % (knob, value))
        run_inverse(p, c, True, "2^16 x 3 %s=%d" % (knob, value))


@pytest.mark.parametrize("seam", [1, 0], ids=["seam-kernel", "two-launches"])
def test_extension_by_two(p, seam):
    """2^16 -> 2^17: lde_seam_kernel (88) in place of the inverse's last and the forward's first pass, or those two passes themselves --
    a MODE 2 last pass and the zero-padded first pass"""
    c = case(16, 3)
    with tuned(p, lde_seam=seam):
        lde = p.ntt_plan(16)["lde"]
        assert lde["seam_fused"] == bool(seam), lde
        d_in, d_out = p.upload(c.x), p.alloc(c.W << 17)
        drain(p)
        p.lde(d_in, d_out, 16, 1, c.W)
        # fused: the forward side runs in sub-chunks of half the chunk's columns (3 columns: one at a time), a seam launch each
        nsub = -(-c.W // max(c.W // 2, 1))
        want = launches(lde["inverse_radix_logs"])[:-1] + ([88] + lde["forward_radix_logs"][1:]) * nsub if seam else launches(digits(p, 16)) + launches(digits(p, 17))
        assert drain(p) == want, "extension: launches"
        same(p.download(d_out, (c.W, 1 << 17)), c.ext, "extension 2^16 x 3 by 2, lde_seam=%d" % seam)
        same(p.download(d_in, c.x.shape), c.x, "extension: input preserved")
        d_in.free()
        d_out.free()
