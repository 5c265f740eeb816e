"""stark/air.py: emit_witness_source -- the generated constraint CHECK on the trace domain (no GPU: the text and the boundary only; what the kernels
compute is tests/test_gpu_witness_inproof.py)."""
import os
import re

import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import build_airs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIRS = sorted(AIR.BUILTIN_AIRS) + ["periodic6"]


def make(name):
    return AIR.periodic_air(6) if name == "periodic6" else AIR.BUILTIN_AIRS[name]()


def walk(e, seen):
    if isinstance(e, AIR.Op):
        walk(e.a, seen)
        walk(e.b, seen)
    else:
        seen.add(e.key())


@pytest.mark.parametrize("name", AIRS)
def test_emitter(name):
    air = make(name)
    before = AIR.emit_quotient_source(air)
    src = AIR.emit_witness_source(air)
    assert src == AIR.emit_witness_source(make(name))                     # deterministic, and a function of the AIR alone
    assert AIR.emit_quotient_source(air) == before                        # the quotient text is what it was
    assert 'extern "C" int %s_witness(' % air.symbol in src and "%s_witness_kernel" % air.symbol in src
    assert "__launch_bounds__(256)" in src and "__shared__" not in src and "template <bool REPORT>" in src
    # only the columns the AIR reads are loaded, each once, current row and next row apart; columns >= W from the stage-2 base
    seen = set()
    for c in air.constraints:
        walk(c, seen)
    cols = {(k[1], k[2]) for k in seen if k[0] == "col"}
    loads = re.findall(r"const u64 c(\d+)(n?) = (trace|s2)\[\(u64\)(\d+) \* N \+ (rr|rn)\];", src)
    assert len(loads) == len(cols) and {(int(i), n == "n") for i, n, _, _, _ in loads} == cols
    for i, n, base, at, row in loads:
        i, at = int(i), int(at)
        assert (base, at) == (("trace", i) if i < air.width else ("s2", i - air.width)) and row == ("rn" if n else "rr")
    fixed = {k[1] for k in seen if k[0] == "fixed"}
    assert {int(i) for i in re.findall(r"const u64 f(\d+) = ", src)} == fixed
    if 0 in fixed:
        assert "const u64 f0 = rr == 0;" in src
    if 1 in fixed:
        assert "const u64 f1 = rr == N - 1;" in src
    # a sparse column: its offset among the periods (zpi_fixed_periods_build's layout, no selectors) and its index mask
    off = 0
    for k, fc in enumerate(air.fixed_cols):
        if 2 + k in fixed:
            assert "const u64 f%d = fixedx[%dULL + (rr & %dULL)];" % (2 + k, off, (1 << fc.lp) - 1) in src
        off += 1 << fc.lp
    # every constraint is reported under its own index, K baked in
    K = len(air.constraints)
    assert [int(k) for k in re.findall(r"zpw_report\(res, %d, (\d+), " % K, src)] == list(range(K))


def test_committed_sources_are_the_emitters():
    """generated/<air>.hip = the quotient text followed by the witness text: build() rewrites nothing"""
    for name, f in AIR.BUILTIN_AIRS.items():
        air = f()
        text = open(os.path.join(build_airs.GEN, name + ".hip")).read()
        assert text == AIR.emit_quotient_source(air) + AIR.emit_witness_source(air), name


def test_error_code_and_binding_table():
    hdr = open(os.path.join(ROOT, "include", "zeth_prover.h")).read()
    assert re.search(r"ZP_ERR_WITNESS\s*=\s*-7\b", hdr) and native.ZP_ERR_WITNESS == -7
    assert "zp_air_witness_fn" in hdr
    for sym in ("zp_stark_set_air_kernel_witness", "zp_stark_prove_witness_report"):
        assert sym in native.SIGNATURES and sym in hdr
    assert issubclass(native.WitnessError, ValueError)
    for method in ("set_air_kernel_witness", "prove_witness_report"):
        assert hasattr(native.Prover, method)
