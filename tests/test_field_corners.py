"""The field primitives under every kernel -- Goldilocks (csrc/gl.hpp, the hand-written forms of csrc/gl_asm.hpp in both scratch windows) and
F_r of BN254 (csrc/fr254.hpp) -- at the operands where a carry, a borrow or a full column shows: tests/native/field_corners.hpp defines them
and the classes they must reach.  Uniformly random operands reach two of the nine product classes; the parity tests elsewhere use those.

Host builds run anywhere (g++, also under the sanitizers: stand-alone programs).  The device programs are built with hipcc for gfx950 and run
as fresh child processes; every comparison is exact, against integer arithmetic."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eigen_zeth_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ARCH", "gfx950")

# the product classes the 518 corner operands reach (borrow class, fold class) -> pairs of E x E; a larger E may only add to them
MUL_CLASS_COUNTS = {"b0,g0": 137578, "b0,G": 103152, "b0,H": 10451, "b1,g0": 1957, "b1,G": 14993, "b1,H": 20, "b2,g0": 33, "b2,G": 136, "b2,H": 4}


def _build_host(exe, include_first=None, extra=()):
    inc = (["-I", include_first] if include_first else []) + ["-I", CSRC]
    subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, *inc, "-o", exe, os.path.join(NATIVE, "gl_host_check.cpp")])


def _report(stdout):
    """'prim NAME cases N mismatches M' and 'class WHAT NAME N' lines -> two dicts"""
    prims = {m[1]: (int(m[2]), int(m[3])) for m in re.finditer(r"^prim (\S+) cases (\d+) mismatches (\d+)$", stdout, re.M)}
    classes = {(m[1], m[2]): int(m[3]) for m in re.finditer(r"^class (\S+) (\S+) (\d+)$", stdout, re.M)}
    return prims, classes


HOST_PRIMS = ["gl_canon", "gl_neg", "gl_add", "gl_sub", "gl_add_weak", "gl_reduce96", "gl_reduce96_weak", "gl_mul", "gl_mul_weak", "gl_sqr",
              "gl_mul_pow2", "gl_acc", "gl_pow", "gl_inv", "e3_mul", "e3_adj", "e3_inv"]


def test_host_primitives_at_every_corner(tmp_path):
    for name, extra in (("plain", ()), ("san", ("-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(tmp_path / ("gl_host_check_" + name))
        _build_host(exe, extra=extra)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
        prims, classes = _report(out.stdout)
        assert sorted(prims) == sorted(HOST_PRIMS)
        assert all(n > 0 and bad == 0 for n, bad in prims.values()), prims
        assert prims["gl_mul"][0] >= 518 * 518 and prims["gl_mul_pow2"][0] >= 95 * 900
        for cls, n in MUL_CLASS_COUNTS.items():
            assert classes[("mul", cls)] >= n, (cls, classes)
        for cls in ("A0", "A1", "A1(s=p)", "A2"):
            assert classes[("add", cls)] > 0, classes
        for cls in ("D0", "D1", "D2"):
            assert classes[("sub", cls)] > 0, classes


# one line of gl.hpp each; every one of them survives 16 million random products (and, below, a million random operands per primitive)
MUTANTS = {
    "reduce96 never takes u without a carry": ("bool cu = (c2 & !bb) | ((bb == c2) & c3);", "bool cu = (c2 & !bb);"),
    "reduce96 adds p after a borrow even with a carry": ("bool cw = bb & !c2;", "bool cw = bb;"),
    "add forgets s in [p, 2^64)": ("return ((s < a) | (u < s)) ? u : s;", "return (s < a) ? u : s;"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_corner_operands_catch_what_random_operands_miss(tmp_path, mutant):
    old, new = MUTANTS[mutant]
    with open(os.path.join(CSRC, "gl.hpp")) as f:
        src = f.read()
    assert src.count(old) == 1, "the line this mutant changes is gone from gl.hpp: " + old
    (tmp_path / "gl.hpp").write_text(src.replace(old, new))
    exe = str(tmp_path / "gl_host_check_mutant")
    _build_host(exe, include_first=str(tmp_path))      # "gl.hpp" resolves to the copy
    corners = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert corners.returncode == 1, corners.stdout[-2000:] + corners.stderr[-2000:]
    m = re.search(r"^total mismatches (\d+)", corners.stdout, re.M)
    assert m and int(m[1]) > 0
    rnd = subprocess.run([exe, "--random", "1000000"], capture_output=True, text=True, timeout=600)
    assert rnd.returncode == 0, rnd.stdout[-2000:] + rnd.stderr[-2000:]
    assert re.search(r"^total mismatches 0 ", rnd.stdout, re.M)
    prims, _ = _report(rnd.stdout)
    assert prims["gl_mul"][0] >= 1000000 and prims["gl_add"][0] >= 1000000      # it did look


# ---------------------------------------------------------------------------------------------------------------- F_r of BN254
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FR_R = 1 << 261                      # the Montgomery radix of fr254.hpp: nine 29-bit limbs
MASK29 = (1 << 29) - 1
OPS = ["add", "sub", "mul", "sqr", "to_mont", "from_mont", "round_trip", "mul3", "u64", "dot1", "dot2", "dot3", "dot4", "dot5", "dot6"]
CASE = np.dtype([("op", "<u4"), ("pad", "<u4"), ("x", "<u4", (6, 9)), ("c", "<u4", (54,)), ("w", "<u8", (4,)),
                 ("r", "<u4", (9,)), ("flag", "<u4"), ("ew", "<u8", (4,))])


def _limbs(v):
    return [(v >> (29 * i)) & MASK29 for i in range(9)]


def _words(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _all_ones_below_r():
    """the value whose nine limbs are all ones as far as it stays below r: eight full limbs under the top limb of r - 1, less one"""
    v = (((R_MOD >> 232) - 1) << 232) | ((1 << 232) - 1)
    assert v < R_MOD and all(l == MASK29 for l in _limbs(v)[:8])
    return v


def fr_operands():
    rinv = pow(FR_R, -1, R_MOD)
    vals = [0, 1, 2, R_MOD - 1, R_MOD - 2, (R_MOD - 1) // 2, FR_R % R_MOD, FR_R * FR_R % R_MOD]
    for k in (28, 29, 30, 58, 87, 232, 253):
        vals += [1 << k, (1 << k) - 1]
    vals.append(_all_ones_below_r())
    rng = random.Random(0xF254)
    vals += [rng.randrange(R_MOD) for _ in range(64)]
    assert all(0 <= v < R_MOD for v in vals)
    return vals, rinv


def write_fr_cases(path):
    """every case with its expected result, by Python integers.  Operands are limb values as the functions take them: fr_mul(a, b) is
    a b / R mod r whatever a and b stand for."""
    vals, rinv = fr_operands()
    nspecial = len(vals) - 64
    rows = []

    def row(op, xs=(), c=(), w=None, r=None, flag=0, ew=None):
        assert r is None or 0 <= r < R_MOD
        rows.append((OPS.index(op), xs, c, w, r, flag, ew))

    for a in vals:
        for b in vals:
            row("add", (a, b), r=(a + b) % R_MOD)
            row("sub", (a, b), r=(a - b) % R_MOD)
            row("mul", (a, b), r=a * b * rinv % R_MOD)
        row("sqr", (a,), r=a * a * rinv % R_MOD)
        row("to_mont", (a,), r=a * FR_R % R_MOD)
        row("from_mont", (a,), r=a * rinv % R_MOD)
        row("round_trip", (a,), r=a)
    for w in vals + [R_MOD, R_MOD + 1, (1 << 256) - 1, (1 << 255), (1 << 256) - (1 << 232)]:
        rows.append((OPS.index("u64"), (), (), w, None, int(w < R_MOD), w))
    rng = random.Random(0x3D07)
    top = [R_MOD - 1, _all_ones_below_r(), R_MOD - 2]
    triples = [(s,) * 6 for s in vals[:nspecial]] + [tuple(rng.choice(top) for _ in range(6)) for _ in range(16)]
    triples += [tuple(rng.choice(vals) for _ in range(6)) for _ in range(256)]
    for t in triples:
        row("mul3", t, r=(t[0] * t[1] + t[2] * t[3] + t[4] * t[5]) * rinv % R_MOD)
    # fr_dotc: N <= 6 products of values below r on limbs below 2^29 -- the bound its comment states (at most 9 N + 9 terms below 2^58 in a
    # column), met with every operand and every constant at its largest; its callers pass table entries, any value below r
    for n in range(1, 7):
        dots = [([x] * n, [c] * n) for x in top for c in top]
        dots += [([rng.choice(top) for _ in range(n)], [rng.choice(top) for _ in range(n)]) for _ in range(8)]
        dots += [([rng.choice(vals) for _ in range(n)], [rng.choice(vals) for _ in range(n)]) for _ in range(64)]
        for xs, cs in dots:
            row("dot%d" % n, xs, cs, r=sum(x * c for x, c in zip(xs, cs)) * rinv % R_MOD)

    rows.sort(key=lambda t: t[0])        # the program wants the cases of an operation together (stable: the order within stays)
    out = np.zeros(len(rows), dtype=CASE)
    for i, (op, xs, c, w, r, flag, ew) in enumerate(rows):
        out["op"][i] = op
        for k, x in enumerate(xs):
            out["x"][i, k] = _limbs(x)
        for k, v in enumerate(c):
            out["c"][i, 9 * k:9 * k + 9] = _limbs(v)
        if w is not None:
            out["w"][i] = _words(w)
            out["r"][i] = _limbs(w)          # fr_from_u64 slices the 256 bits it is given
            out["ew"][i] = _words(ew)
        else:
            out["r"][i] = _limbs(r)
        out["flag"][i] = flag
    assert CASE.itemsize == 544
    out.tofile(path)
    return len(rows)


def _check_fr(exe, cases, ncases):
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    prims, _ = _report(out.stdout)
    assert len(prims) == len(OPS) and sum(n for n, _ in prims.values()) == ncases
    assert all(n > 0 and bad == 0 for n, bad in prims.values()), prims
    return out.stdout


def test_fr254_host_at_corners(tmp_path):
    cases = str(tmp_path / "fr_cases.bin")
    n = write_fr_cases(cases)
    for name, extra in (("plain", ()), ("san", ("-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"))):
        exe = str(tmp_path / ("fr254_check_" + name))
        subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-I", CSRC, "-x", "c++", os.path.join(NATIVE, "fr254_check.hip"), "-o", exe])
        assert "build host" in _check_fr(exe, cases, n)


# ---------------------------------------------------------------------------------------------------------------- on the GPU
_LATCH = {"dead": None}       # one for the whole session: tests/test_fq254.py starts its device program through it as well


def run_latched(key, argv, timeout=120):
    """start a device program as a fresh child; after one dies of a signal, runs out of time or reports a HIP error nothing more is started"""
    if _LATCH["dead"]:
        pytest.fail("not started: " + _LATCH["dead"])
    try:
        out = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _LATCH["dead"] = "%s ran out of time" % key
        pytest.fail(_LATCH["dead"])
    if out.returncode < 0 or out.returncode >= 2:
        _LATCH["dead"] = "%s ended with status %d: %s" % (key, out.returncode, out.stderr[-1000:])
        pytest.fail(_LATCH["dead"] + out.stdout[-2000:])
    return out


class _Device:
    """the three programs, built once; they are started through run_latched"""

    def __init__(self, d):
        self.exe = {}
        flags = ["-O3", "-std=c++17", "--offload-arch=" + ARCH, "-I", CSRC]
        for window in (116, 52):
            self.exe[window] = os.path.join(d, "gl_device_check_%d" % window)
            subprocess.check_call([HIPCC, *flags, "-DGL_ASM_SCRATCH_BASE=%d" % window, "-o", self.exe[window], os.path.join(NATIVE, "gl_device_check.hip")])
        self.exe["fr"] = os.path.join(d, "fr254_check_device")
        subprocess.check_call([HIPCC, *flags, "-o", self.exe["fr"], os.path.join(NATIVE, "fr254_check.hip")])
        self.cases = os.path.join(d, "fr_cases.bin")
        self.ncases = write_fr_cases(self.cases)

    def run(self, key, *args):
        return run_latched(key, [self.exe[key], *args])


@pytest.fixture(scope="module")
def device_checks(tmp_path_factory):
    return _Device(str(tmp_path_factory.mktemp("field_corners")))


DEVICE_PRIMS = ["gl_mul2.slot1", "gl_mul2.slot2", "gl_mul2w.slot1", "gl_mul2w.slot2", "gl_mul1", "gl_mul1w", "gl_mul", "gl_add", "gl_sub",
                "gl_bfly2.slot_a", "gl_bfly2.slot_b", "gl_shl12", "gl_mul_pow2", "gl_acc.sequences", "gl_acc.wrap_counters", "gl_acc_reduce.states"]


@pytest.mark.gpu
@pytest.mark.parametrize("window", [116, 52])
def test_device_primitives_at_every_corner(device_checks, window):
    out = device_checks.run(window)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert "window %d " % window in out.stdout
    prims, classes = _report(out.stdout)
    assert sorted(prims) == sorted(DEVICE_PRIMS)
    assert all(n > 0 and bad == 0 for n, bad in prims.values()), prims
    for what in ("gl_mul2.slot1", "gl_mul2.slot2", "gl_mul2w.slot1", "gl_mul2w.slot2", "gl_mul1", "gl_mul1w", "gl_mul"):
        for cls, n in MUL_CLASS_COUNTS.items():
            assert classes[(what, cls)] >= n, (what, cls)
    for what in ("gl_bfly2.slot_a", "gl_bfly2.slot_b"):
        for cls in ("A0", "A1", "A1(s=p)", "A2", "D0", "D1", "D2"):
            assert classes[(what, cls)] > 0, (what, cls)


@pytest.mark.gpu
def test_fr254_device_at_corners(device_checks):
    out = device_checks.run("fr", device_checks.cases)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert "build device" in out.stdout
    prims, _ = _report(out.stdout)
    assert len(prims) == len(OPS) and sum(n for n, _ in prims.values()) == device_checks.ncases
    assert all(n > 0 and bad == 0 for n, bad in prims.values()), prims
