"""NTT / LDE on the GPU: every root class, every launch-shaping knob and every chunk seam, bit-exact against the CPU oracle.

Why: csrc/ntt.hip chooses one of ~110 kernel instantiations per pass (zpi_pass_shape -> dispatch_pass -> launch_pass2 ->
pick_pass_kernel) and the user's root enters the shift-only butterflies only as j0inv, an odd residue mod 16 that renames
outputs (exchange2, exchange2_l4, the per-lane chain's jr, the limb tables' rot, the seam kernel's j0inv_i / j0inv_f).  The
default root is class 5 forward and 11 inverse; a wrong mask or rotation that keeps those two right is invisible at the default
root.  ROOT32_DEFAULT^k, k = 1, 3 .. 15, gives eight roots that cover the eight classes in each direction
(tests/test_ntt_root_classes.py pins the oracle at them on the CPU).

Every run also reads the launch sequence back (set_profiling / pass_timings: -L a first pass, L a later pass, 88 the seam
kernel) and compares it with what the plan and the column chunking imply, so a case cannot pass on another route than it claims.

Shape (A1,A2,A3,logT) of dispatch_pass  <- radix, knob               first pass (table / chain, padded or not)       later pass (MODE 0 / 1 / 2)
  (3,2,0,5)  L=5                                                      test_B_maxl (chain: L < 7 has no table)         test_B_maxl
  (3,3,0,5)  L=6                                                      test_B_maxl                                      test_A_large[three-7x6x6], test_B_maxl
  (4,3,0,5)  L=7                                                      test_A_small[*-7x7] (chain: 4 tiles), test_A_large[three-7x6x6] (table), test_B_order[23-1-2]
                                                                                                                       test_A_small[*-8x7], test_A_large[three-8x7x7]
  (4,4,0,4)  L=8                                                      test_A_small[table-8x*, chain-8x*]               test_A_small[*-8x8], test_A_seam (two-launch)
  (4,4,0,5)  L=8, ntt_logt=5                                          test_B_logt5 (padded: the extensions)            test_B_logt5 (MODE 2 at 2^16)
  (3,3,3,4)  L=9                                                      test_A_small[r512-9x9], test_B_order[17-3-1]       test_A_small[r512-*]
  (3,3,3,5)  L=9, ntt_logt9=5                                         test_B_logt9[18]                                 test_B_logt9
  (4,3,3,4)  L=10, ntt_maxl=10                                        test_A_large[maxl10]                             test_A_large[maxl10]
  (4,4,3,3)  L=11, ntt_maxl=11                                        test_A_large[maxl11]                             test_A_large[maxl11, maxl12]
  (4,4,4,2)  L=12, ntt_maxl=12                                        test_A_large[maxl12]                             test_A_large[maxl12] (extension), test_B_logt12 (multiplying)
  (4,4,4,1)  L=12, ntt_logt12=1                                       test_B_logt12                                    test_B_logt12 (forward last pass)
  (4,3,0,5,BIG), (4,4,0,4,BIG): above 2^28 rows, out of this module's size limit (tests/test_gpu_parity_large.py, 2^29).
Other selectors of pick_pass_kernel / launch_pass2 / lde_route:
  limb butterflies (ntt_limb=1, L <= 8, table first pass)             test_A_small[limb-8x8], test_A_large[limb-8x7x7], test_B_logt5
  per-lane chain (ntt_tw1=0, or a grid that is no multiple of 8)      test_A_small[chain-*]
  lde_seam_kernel (88), with / without the coefficient store          test_A_seam, test_B_seam_tpw, test_C_chunks
  two-launch extension (padded first pass, MODE 2 last pass)          test_A_seam, test_A_blowup4, test_C_chunks and every default extension below 2^16
  tiles per workgroup ntt_tpw / seam_tpw                              test_B_tpw, test_B_seam_tpw
  digit order ntt_order                                               test_B_order
  4 and 5 passes (both scratch buffers alternate)                     test_B_maxl
  columns per launch ntt_chunk_log (c0, h0, wf, ragged ends)          test_C_chunks
  a radix below 2^5                                                   test_B_unsupported_radix

The module owns its context (fixture `p`): no knob or root set here can leak into the session's shared one, every knob and the
root are still restored in `finally` (tuned), and the last test checks that nothing was left changed.  Knob defaults are read
from csrc/ctx.hpp.  Data: O.random_field by seed, with 0, P-1, 1 and 2^32 in front.  Buffers stay <= 2^25 elements."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.native import ZpError
from oracle import oracle as O

pytestmark = pytest.mark.gpu
P = O.P
ROOTS = {k: pow(native.ROOT32_DEFAULT, k, P) for k in range(1, 16, 2)}
ALL_K = tuple(ROOTS)
HALF_K = (1, 3, 5, 7)        # forward classes 5, 7, 1, 3 and inverse classes 11, 9, 15, 13: all eight between them
ODD16 = set(range(1, 16, 2))

KNOBS = ("ntt_logt", "ntt_tpw", "ntt_logt9", "ntt_logt12", "ntt_tw1", "ntt_limb", "ntt_maxl", "ntt_order", "ntt_chunk_log",
         "lde_seam", "lde_seam_plans", "seam_tpw")
_FIELD = {"ntt_logt": "logt", "ntt_tpw": "tpw", "ntt_logt9": "logt9", "ntt_logt12": "logt12"}   # zp_set_tuning key -> zp_ctx::tune_<field>


def _defaults():
    with open(os.path.join(os.path.dirname(native.__file__), "csrc", "ctx.hpp")) as f:
        found = dict(re.findall(r"\btune_(\w+) = (-?\d+)", f.read()))
    return {k: int(found[_FIELD.get(k, k)]) for k in KNOBS}


DEFAULTS = _defaults()
_now = dict(DEFAULTS, root=native.ROOT32_DEFAULT)       # what the module's context is set to


@pytest.fixture(scope="module")
def p():
    pr = native.Prover(0)
    pr.set_profiling(True)
    yield pr
    pr.close()


@contextlib.contextmanager
def tuned(p, root=None, **knobs):
    """set tuning knobs (and the root) on the context; put back what was there before, whatever happens inside"""
    before = {k: _now[k] for k in knobs}
    root_before = _now["root"]
    try:
        for k, v in knobs.items():
            p.set_tuning(k, v)
            _now[k] = v
        if root is not None:
            p.set_constants(native.ZP_CONST_ROOT32, [root])
            _now["root"] = root
        yield
    finally:
        for k, v in before.items():
            p.set_tuning(k, v)
            _now[k] = v
        p.set_constants(native.ZP_CONST_ROOT32, [root_before])
        _now["root"] = root_before


def j0inv(root32, inverse):
    """the search of zpi_get_plan_role: j with (2^12)^j == w_16, then j^-1 mod 16"""
    w16 = pow(root32, 1 << 28, P)
    if inverse:
        w16 = pow(w16, P - 2, P)
    (j,) = [j for j in range(1, 16, 2) if pow(1 << 12, j, P) == w16]
    return pow(j, -1, 16)


def test_roots_cover_every_class_each_way():
    assert {j0inv(r, False) for r in ROOTS.values()} == ODD16 and {j0inv(r, True) for r in ROOTS.values()} == ODD16
    assert {j0inv(ROOTS[k], inv) for k in HALF_K for inv in (False, True)} == ODD16
    assert (j0inv(ROOTS[1], False), j0inv(ROOTS[1], True)) == (5, 11)


# ---- inputs and oracle results, made once per (size, width, root)
class Case:
    def __init__(self, logn, W, k):
        self.logn, self.W, self.k, self.root = logn, W, k, ROOTS[k]
        self.x = O.random_field((W, 1 << logn), 9000 + 64 * logn + 16 * W + k)
        self.x[0, :4] = np.array([0, P - 1, 1, 2 ** 32], dtype=np.uint64)
        self._ext = {}

    @functools.cached_property
    def fwd(self):
        return O.ntt(self.x, self.root)

    @functools.cached_property
    def inv(self):
        return O.intt(self.x, self.root)

    def ext(self, logb, shift):
        if (logb, shift) not in self._ext:
            self._ext[logb, shift] = O.lde(self.x, logb, shift, self.root)
        return self._ext[logb, shift]

    @functools.cached_property
    def coef(self):
        """O.intt(x, root)[i] * shift^i, the whole column"""
        return O.coset_scaled_coefficients(self.x, O.SHIFT_DEFAULT, self.root)


@functools.lru_cache(maxsize=4)
def case(logn, W, k=1):
    return Case(logn, W, k)


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d elements differ, first at (column, row) %s" % (what, len(bad), got.size, tuple(bad[0])))


# ---- the launches a call must make, from the plan and the chunking
def digits(p, logn):
    return [q["radix_log"] for q in p.ntt_plan(logn)["passes"]]


def launches(d):
    return [-d[0]] + list(d[1:])


def chunks(logn, W):
    """columns per launch (chunk_columns) and the chunk widths of W columns"""
    wc = min(max((1 << (_now["ntt_chunk_log"] or 28)) >> logn, 1), W)
    return wc, [min(wc, W - c0) for c0 in range(0, W, wc)]


def expect_ntt(p, logn, W):
    return launches(digits(p, logn)) * len(chunks(logn, W)[1])


def expect_lde(p, logn, logb, W, coef):
    """(launch sequence, fused) of zp_lde: lde_route / lde_fused / the two-launch loop of zpi_lde"""
    plan = p.ntt_plan(logn)["lde"]         # the route without a coefficient store
    fused = logb == 1 and plan["seam_fused"] and (not coef or _now["lde_seam"] == 2)
    wc, ws = chunks(logn, W)
    if not fused:      # per chunk two calls of zpi_ntt_run, each chunking its w columns again by its own size
        seq = []
        for w in ws:
            seq += launches(digits(p, logn)) * len(chunks(logn, w)[1]) + launches(digits(p, logn + logb)) * len(chunks(logn + logb, w)[1])
        return seq, False
    wf = max(wc // 2, 1)
    seq = []
    for w in ws:
        seq += launches(plan["inverse_radix_logs"])[:-1]
        for _ in range(0, w, wf):
            seq += [88] + plan["forward_radix_logs"][1:]
    return seq, True


def drain(p):
    return [r for r, _ in p.pass_timings()]


# ---- one call each, compared over every element
def check_forward(p, c, inplace=False):
    W, logn = c.W, c.logn
    d_in = p.upload(c.x)
    d_out = d_in if inplace else p.alloc(W << logn)
    drain(p)
    p.ntt(d_in, d_out, logn, W)
    assert drain(p) == expect_ntt(p, logn, W), "forward 2^%d x %d: launches" % (logn, W)
    same(p.download(d_out, c.x.shape), c.fwd, "forward 2^%d x %d k=%d %s" % (logn, W, c.k, "in place" if inplace else "out of place"))
    if not inplace:
        same(p.download(d_in, c.x.shape), c.x, "forward: input preserved")
        d_out.free()
    d_in.free()


def check_inverse(p, c, inplace=True):
    """up to 2^18 rows iNTT(x) against O.intt(x); above, iNTT(O.ntt(x)) against x (one oracle transform less per case:
    O.intt(O.ntt(x)) == x is tests/test_oracle.py's and O.ntt(x) is as random an input as x)"""
    W, logn = c.W, c.logn
    src, want = (c.x, c.inv) if logn <= 18 else (c.fwd, c.x)
    d_in = p.upload(src)
    d_out = d_in if inplace else p.alloc(W << logn)
    drain(p)
    p.intt(d_in, d_out, logn, W)
    assert drain(p) == expect_ntt(p, logn, W), "inverse 2^%d x %d: launches" % (logn, W)
    same(p.download(d_out, c.x.shape), want, "inverse 2^%d x %d k=%d" % (logn, W, c.k))
    if not inplace:
        d_out.free()
    d_in.free()


def check_lde(p, c, logb=1, coef=False, fused=None):
    """zp_lde with the default shift against O.lde; with coef, the coefficient store against O.intt(x) * shift^i"""
    W, logn = c.W, c.logn
    what = "extension 2^%d x %d by %d k=%d%s" % (logn, W, 1 << logb, c.k, " + coefficients" if coef else "")
    d_in = p.upload(c.x)
    d_out = p.alloc(W << (logn + logb))
    d_coef = p.alloc(W << logn) if coef else None
    seq, is_fused = expect_lde(p, logn, logb, W, coef)
    if fused is not None:
        assert is_fused == fused, what + ": route"
    drain(p)
    p.lde(d_in, d_out, logn, logb, W, d_coef=d_coef)
    assert drain(p) == seq, what + ": launches"
    same(p.download(d_out, (W, 1 << (logn + logb))), c.ext(logb, O.SHIFT_DEFAULT), what)
    if coef:
        same(p.download(d_coef, c.x.shape), c.coef, what + ": coefficient store")
        d_coef.free()
    same(p.download(d_in, c.x.shape), c.x, what + ": input preserved")
    d_in.free()
    d_out.free()


def check_three(p, c, lde_case=None):
    """forward out of place, inverse in place, extension by 2 with the default shift"""
    check_forward(p, c)
    check_inverse(p, c)
    check_lde(p, lde_case or c)


def lde_case_of(c):
    """the extension of a 2^25-row case runs on 2^24 rows: its output is the largest buffer allowed here, and its zero-padded
    forward transform has the case's own size and plan"""
    return c if c.logn <= 24 else case(24, c.W, c.k)


# =====================================================================================================================
# A. eight root classes x every kernel form that reads j0inv
# =====================================================================================================================
# id, logn, knobs, radix logs of the forward plan, first_pass_table, lde.seam_fused
SMALL_FORMS = [
    ("table-7x7", 14, {}, [7, 7], True, False),
    ("table-8x7", 15, {}, [8, 7], True, False),
    ("table-8x8", 16, {}, [8, 8], True, True),
    ("chain-7x7", 14, {"ntt_tw1": 0}, [7, 7], False, False),
    ("chain-8x7", 15, {"ntt_tw1": 0}, [8, 7], False, False),
    ("chain-8x8", 16, {"ntt_tw1": 0}, [8, 8], False, False),
    ("r512-8x9", 17, {}, [8, 9], True, False),
    ("r512-9x9", 18, {}, [9, 9], False, False),
    ("limb-8x8", 16, {"ntt_limb": 1}, [8, 8], True, True),
]
LARGE_FORMS = [
    ("three-7x6x6", 19, 2, {}, [7, 6, 6], True, False),
    ("maxl10", 20, 2, {"ntt_maxl": 10}, [10, 10], False, False),
    ("maxl11", 21, 2, {"ntt_maxl": 11}, [11, 10], False, False),
    ("three-8x7x7", 22, 2, {}, [8, 7, 7], True, True),
    ("limb-8x7x7", 22, 2, {"ntt_limb": 1}, [8, 7, 7], True, True),
    ("maxl12", 23, 1, {"ntt_maxl": 12}, [12, 11], False, False),
]


def assert_form(p, logn, passes, table, seam):
    plan = p.ntt_plan(logn)
    assert [q["radix_log"] for q in plan["passes"]] == passes, plan
    assert plan["first_pass_table"] == table, plan
    assert plan["lde"]["seam_fused"] == seam, plan
    for q in plan["passes"]:
        assert (q["rounds"][2] != 0) == (q["radix_log"] >= 9), plan      # three register rounds from radix 512 up
    return plan


@pytest.mark.parametrize("form,k", [(f, k) for f in SMALL_FORMS for k in ALL_K], ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_A_small(p, form, k):
    """2^14 .. 2^18 rows x 3 columns: every form x all eight roots (forward class, inverse class) -- forward out of place,
    inverse in place, extension by 2.  At 2^14 the plan names the table but the first pass has 4 tiles, no multiple of the 8
    XCDs, and launch_pass2 takes the per-lane chain; the table form of a radix-128 first pass runs in test_A_large[three-7x6x6]"""
    _, logn, knobs, passes, table, seam = form
    c = case(logn, 3, k)
    with tuned(p, root=c.root, **knobs):
        assert_form(p, logn, passes, table, seam)
        check_three(p, c)


@pytest.mark.parametrize("form,k", sorted([(f, k) for f in LARGE_FORMS for k in HALF_K], key=lambda v: (v[0][1], v[1])),
                         ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_A_large(p, form, k):
    """three-pass plans, the limb form at 2^22 and the radix 2^10 .. 2^12 passes: four roots whose forward and inverse
    classes are the eight between them"""
    _, logn, W, knobs, passes, table, seam = form
    c = case(logn, W, k)
    with tuned(p, root=c.root, **knobs):
        assert_form(p, logn, passes, table, seam)
        check_three(p, c)


@pytest.mark.parametrize("k", ALL_K)
@pytest.mark.parametrize("logn,W,inv_digits,fwd_digits", [(16, 3, [8, 8], [8, 9]), (21, 2, [7, 6, 8], [8, 7, 7])])
def test_A_seam(p, logn, W, inv_digits, fwd_digits, k):
    """lde_seam_kernel (j0inv_i of 2^logn rows, j0inv_f of 2^(logn+1) rows) on the default plans (2^16) and on the seam-role
    plans (2^21), with and without the coefficient store; and the two-launch extension of the same columns"""
    c = case(logn, W, k)
    with tuned(p, root=c.root, lde_seam=2):
        lde = p.ntt_plan(logn)["lde"]
        assert lde["seam_fused"] and lde["inverse_radix_logs"] == inv_digits and lde["forward_radix_logs"] == fwd_digits, lde
        assert (j0inv(c.root, True), j0inv(c.root, False)) == {1: (11, 5), 3: (9, 7), 5: (15, 1), 7: (13, 3), 9: (3, 13), 11: (1, 15),
                                                                 13: (7, 9), 15: (5, 11)}[k]
        check_lde(p, c, fused=True)
        check_lde(p, c, coef=True, fused=True)
    with tuned(p, root=c.root, lde_seam=0):
        assert not p.ntt_plan(logn)["lde"]["seam_fused"]
        check_lde(p, c, fused=False)
        check_lde(p, c, coef=True, fused=False)


@pytest.mark.parametrize("k", ALL_K)
def test_A_blowup4(p, k):
    c = case(14, 3, k)
    with tuned(p, root=c.root):
        assert digits(p, 14) == [7, 7] and digits(p, 16) == [8, 8]
        check_lde(p, c, logb=2, fused=False)
        check_lde(p, c, logb=2, coef=True, fused=False)


# =====================================================================================================================
# B. the launch-shaping knobs
# =====================================================================================================================
@pytest.mark.parametrize("logn,W,passes", [(17, 3, [8, 9]), (18, 3, [9, 9]), (25, 1, [8, 8, 9])], ids=["17", "18", "25"])
def test_B_logt9(p, logn, W, passes):
    """ntt_logt9 = 5: shape (3,3,3,5), a 128 KiB tile of 32 columns on 1024 threads -- as a chain first pass (2^18), a plain and
    a multiplying last pass, and behind a zero-padded first pass"""
    c = case(logn, W)
    with tuned(p, ntt_logt9=5):
        plan = p.ntt_plan(logn)
        assert [q["radix_log"] for q in plan["passes"]] == passes, plan
        for q in plan["passes"]:
            assert q["tile"] == (32 if q["radix_log"] == 9 else 16) and q["rounds"] == ([3, 3, 3] if q["radix_log"] == 9 else [4, 4, 0]), plan
        check_three(p, c, lde_case_of(c))


@pytest.mark.parametrize("logn,passes,tiles", [(24, [12, 12], [2, 2]), (23, [12, 11], [2, 8])], ids=["24", "23"])
def test_B_logt12(p, logn, passes, tiles):
    """ntt_logt12 = 1 with ntt_maxl = 12: shape (4,4,4,1), 64 KiB tiles of 2 columns, for a first pass and a plain last pass.
    A multiplying last pass (the inverse transform, the inverse side of an extension) stays on (4,4,4,2): the plan JSON is the
    forward plan only, so that per-direction tile (2 against 4) is not visible in it -- what covers it is that the inverse
    transform and the extension, which run it, are correct"""
    c = case(logn, 1)
    with tuned(p, ntt_maxl=12, ntt_logt12=1):
        plan = p.ntt_plan(logn)
        assert [q["radix_log"] for q in plan["passes"]] == passes and [q["tile"] for q in plan["passes"]] == tiles, plan
        assert not plan["lde"]["seam_fused"]
        check_three(p, c)
    assert [q["tile"] for q in p.ntt_plan(logn)["passes"]] != tiles


def test_B_logt5(p):
    """ntt_logt = 5: radix-256 passes on 32-column tiles, shape (4,4,0,5) -- unpadded and zero-padded table first pass, MODE 1
    and MODE 2 last pass, and all of them on limbs.  The seam kernel is built for 16-column tiles: no fused route"""
    with tuned(p, ntt_logt=5):
        plan = p.ntt_plan(16)
        assert plan["first_pass_table"] and [q["tile"] for q in plan["passes"]] == [32, 32] and not plan["lde"]["seam_fused"], plan
        assert p.ntt_plan(15)["passes"][0] == {"radix_log": 8, "rounds": [4, 4, 0], "tile": 32}
        for logn in (15, 16):          # extensions 2^15 -> 2^16 (8,7 then padded 8,8) and 2^16 -> 2^17 (8,8 then padded 8,9)
            c = case(logn, 3)
            check_three(p, c)
            check_lde(p, c, coef=True, fused=False)
        with tuned(p, ntt_limb=1):
            check_three(p, case(16, 3))
            with tuned(p, root=ROOTS[7]):       # limb rot at classes 3 / 13 on the wide tile
                check_three(p, case(16, 3, 7))
    assert p.ntt_plan(16)["lde"]["seam_fused"]


def surviving_tpw(tpw, tiles, W, cus):
    """the loop of launch_pass2"""
    while tpw > 1 and (tiles % tpw != 0 or tiles // tpw * W < 4 * cus):
        tpw >>= 1
    return tpw


@pytest.mark.parametrize("tpw", [1, 2, 4, 3])
def test_B_tpw(p, tpw):
    """ntt_tpw: tiles per workgroup.  2^20 rows x 32 (16 for the extension, whose output is then 2^25 elements): the passes
    have 256 (radix 128, 32-column tiles) and 512 (radix 64) tiles, so 4 survives the loop of launch_pass2 on every pass;
    2^16 x 3 has 16 tiles a pass and every value is cut back to 1.  3 divides no tile count: it must run as 1"""
    cus = p.device_info()["cus"]
    want = {1: 1, 2: 2, 4: 4, 3: 1}[tpw]
    with tuned(p, ntt_tpw=tpw):
        assert digits(p, 20) == [7, 7, 6] and digits(p, 21) == [7, 7, 7] and digits(p, 16) == [8, 8]
        for tiles, W in ((256, 32), (512, 32), (256, 16), (512, 16)):      # (2^20 / 128) / 32 ..; the extension's forward side is 2^21 / 128 / 32 = 512
            assert surviving_tpw(tpw, tiles, W, cus) == want, (tiles, W, cus)
        assert surviving_tpw(tpw, 16, 3, cus) == 1
        c = case(20, 32)
        check_forward(p, c)
        check_inverse(p, c)
        check_lde(p, case(20, 16))
        check_three(p, case(16, 3))


@pytest.mark.parametrize("tpw", [1, 4])
def test_B_seam_tpw(p, tpw):
    """seam_tpw = 1, 4: inverse tiles per workgroup of the seam kernel.  Its grid must stay a multiple of 8 workgroups a
    column: at 2^16 rows (16 tiles) 4 leaves 4 workgroups and the route must fall back to two launches.  2^17 rows have no
    fused route at any value (the inverse plan (8,9) does not end in radix 256 and no seam-role plan exists below three passes)"""
    with tuned(p, seam_tpw=tpw):
        for logn, fused in ((16, tpw == 1), (17, False), (21, True), (22, True)):
            c = case(logn, 2)
            assert p.ntt_plan(logn)["lde"]["seam_fused"] == fused, (logn, tpw)
            check_lde(p, c, fused=fused)
            with tuned(p, lde_seam=2):
                check_lde(p, c, coef=True, fused=fused)


ORDERED = {15: ([8, 7], [7, 8]), 17: ([9, 8], [8, 9]), 22: ([8, 7, 7], [7, 7, 8]), 23: ([8, 8, 7], [7, 8, 8]), 25: ([9, 8, 8], [8, 8, 9])}


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("logn,W", [(15, 3), (17, 3), (22, 2), (23, 1), (25, 1)])
def test_B_order(p, logn, W, order):
    """ntt_order = 1 (larger digits first: a radix-512 first pass on the per-lane chain at 2^17 and 2^25) and 2 (larger digits
    last: a radix-128 first pass in front of radix-256 passes at 2^22 / 2^23)"""
    c = case(logn, W)
    with tuned(p, ntt_order=order):
        plan = p.ntt_plan(logn)
        assert [q["radix_log"] for q in plan["passes"]] == ORDERED[logn][order - 1], plan
        assert plan["first_pass_table"] == (plan["passes"][0]["radix_log"] != 9), plan
        check_three(p, c, lde_case_of(c))


@pytest.mark.parametrize("maxl,logn,W,ks,passes,lde_logn,lde_inv,lde_fwd", [
    (7, 22, 2, (1,), [6, 6, 5, 5], 22, [6, 6, 5, 5], [6, 6, 6, 5]),          # L=6 first pass, unpadded and padded
    (6, 20, 2, HALF_K, [5, 5, 5, 5], 20, [5, 5, 5, 5], [6, 5, 5, 5]),        # L=5 first pass at every class
    (6, 25, 1, (1,), [5, 5, 5, 5, 5], 24, [6, 6, 6, 6], [5, 5, 5, 5, 5]),    # five passes; L=5 first pass, unpadded and padded
    (8, 25, 1, (1,), [7, 6, 6, 6], 24, [8, 8, 8], [7, 6, 6, 6]),
], ids=["7-22", "6-20", "6-25", "8-25"])
def test_B_maxl(p, maxl, logn, W, ks, passes, lde_logn, lde_inv, lde_fwd):
    """ntt_maxl = 8, 7, 6: plans of four and five passes (the two scratch buffers alternate: by default only from 2^28 rows
    up), radix-32 passes -- shape (3,2,0,5), in no default plan -- and radix-32 / radix-64 first passes on a full and on a
    zero-padded column"""
    for k in ks:
        c = case(logn, W, k)
        with tuned(p, root=c.root, ntt_maxl=maxl):
            plan = p.ntt_plan(logn)
            assert [q["radix_log"] for q in plan["passes"]] == passes and plan["first_pass_table"] == (passes[0] >= 7), plan
            assert digits(p, lde_logn) == lde_inv and digits(p, lde_logn + 1) == lde_fwd
            assert not p.ntt_plan(lde_logn)["lde"]["seam_fused"]
            check_three(p, c, c if lde_logn == logn else case(lde_logn, W, k))


def test_B_unsupported_radix(p):
    """ntt_maxl = 6 at 2^13 rows is (5,4,4): no radix-16 pass is built, the call must say so and the context must go on working"""
    c = case(13, 3)
    d = p.upload(c.x)
    with tuned(p, ntt_maxl=6):
        assert digits(p, 13) == [5, 4, 4]
        with pytest.raises(ZpError, match="unsupported pass radix"):
            p.ntt(d, d, 13, 3)
    d.free()
    p.sync()
    assert digits(p, 13) == [7, 6]
    check_three(p, c)


# =====================================================================================================================
# C. chunk seams at small sizes, every element compared
# =====================================================================================================================
@pytest.mark.parametrize("logn,W,chunk_log,wc,widths", [
    (16, 7, 18, 4, [4, 3]),            # wf = 2: sub-chunks 2+2 and 2+1 (ragged chunk, ragged sub-chunk)
    (16, 3, 17, 2, [2, 1]),            # wf = 1
    (16, 3, 16, 1, [1, 1, 1]),
    (16, 3, 12, 1, [1, 1, 1]),         # 2^12 >> 16 = 0 columns: one at a time
    (21, 5, 23, 4, [4, 1]),            # seam-role plans (7,6,8) + (8,7,7)
    (21, 5, 22, 2, [2, 2, 1]),
    (21, 5, 21, 1, [1, 1, 1, 1, 1]),
], ids=["16x7-18", "16x3-17", "16x3-16", "16x3-12", "21x5-23", "21x5-22", "21x5-21"])
def test_C_chunks(p, logn, W, chunk_log, wc, widths):
    """ntt_chunk_log makes the chunks small: the column offsets c0 * in_valid (padded input), (c0 + h0) * N (coefficient
    store across chunk and sub-chunk boundaries), the forward sub-chunks wf = wc / 2 of lde_fused and the scratch sizing --
    forward in place and out of place, inverse, the fused and the two-launch extension with and without the coefficient
    store, blow-up 4.  The launch counts must be the chunked ones"""
    c = case(logn, W)
    with tuned(p, ntt_chunk_log=chunk_log):
        assert chunks(logn, W) == (wc, widths)
        nsub = sum(-(-w // max(wc // 2, 1)) for w in widths)
        check_forward(p, c, inplace=True)
        check_forward(p, c, inplace=False)
        check_inverse(p, c, inplace=True)
        check_inverse(p, c, inplace=False)
        with tuned(p, lde_seam=2):
            for coef in (False, True):
                seq, fused = expect_lde(p, logn, 1, W, coef)
                assert fused and seq.count(88) == nsub and len(seq) == (len(digits(p, logn)) - 1) * len(widths) + len(digits(p, logn + 1)) * nsub
                check_lde(p, c, coef=coef, fused=True)
        with tuned(p, lde_seam=0):
            for coef in (False, True):
                seq, _ = expect_lde(p, logn, 1, W, coef)
                # first passes: one inverse per chunk, and the zero-padded forward side in chunks of half as many columns (2N rows each)
                assert sum(r < 0 for r in seq) == len(widths) + nsub
                check_lde(p, c, coef=coef, fused=False)
        c4 = c if logn == 16 else case(logn, 3)       # 2^23 x 3 outputs: within the buffer limit
        assert len(chunks(logn, c4.W)[1]) >= (2 if chunk_log < 23 else 1)
        check_lde(p, c4, logb=2, fused=False)
        check_lde(p, c4, logb=2, coef=True, fused=False)


# =====================================================================================================================
def test_Z_no_knob_and_no_root_left_changed(p):
    assert _now == dict(DEFAULTS, root=native.ROOT32_DEFAULT)
    assert int(p.get_constants(native.ZP_CONST_ROOT32, 1)[0]) == native.ROOT32_DEFAULT
    fresh = native.Prover(0)
    try:
        for logn in (16, 22):
            assert p.ntt_plan(logn) == fresh.ntt_plan(logn), logn
        x = case(16, 3).x
        d = fresh.upload(x)
        fresh.ntt(d, d, 16, 3)
        want = fresh.download(d, x.shape)
    finally:
        fresh.close()
    d = p.upload(x)
    p.ntt(d, d, 16, 3)
    same(p.download(d, x.shape), want, "module context against a fresh one")
    same(want, case(16, 3).fwd, "fresh context against the oracle")
