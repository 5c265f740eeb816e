"""Generates and compiles the constraint kernels of the built-in AIRs for gfx950:
generated/<air>.hip + generated/<air>_witness_rows.hip -> generated/libzpair_<air>.so (AIR plug-in ABI, include/zeth_prover.h)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GEN = os.path.join(HERE, "generated")
CSRC = os.path.join(os.path.dirname(HERE), "csrc")


def _stem(air):
    """built-in AIRs: their name.  AIRs made per shape (the verifier AIRs of the recursion layers: one name, many statements): name + digest"""
    return air.name + ("_" + air.digest() if air.fixed_cols else "")


def lib_path(air):
    return os.path.join(GEN, "libzpair_%s.so" % _stem(air))


def _write(path, code, force):
    if force or not os.path.exists(path) or open(path).read() != code:
        with open(path, "w") as f:
            f.write(code)
    return path


def build_air(air, force=False):
    from .air import emit_quotient_source, emit_witness_source, emit_witness_rows_source
    os.makedirs(GEN, exist_ok=True)
    # one library, four symbols: <symbol>, <symbol>_rows, <symbol>_witness from <stem>.hip; <symbol>_witness_rows from a file of its own
    srcs = [_write(os.path.join(GEN, _stem(air) + ".hip"), emit_quotient_source(air, "hip") + emit_witness_source(air), force),
            _write(os.path.join(GEN, _stem(air) + "_witness_rows.hip"), emit_witness_rows_source(air), force)]
    out = lib_path(air)
    if force or not os.path.exists(out) or os.path.getmtime(out) < max([os.path.getmtime(s) for s in srcs] + [os.path.getmtime(os.path.join(CSRC, "gl.hpp"))]):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                               "-I", CSRC, "-o", out] + srcs)
    return out


def build_all(force=False):
    from .air import BUILTIN_AIRS
    return [build_air(f(), force) for f in BUILTIN_AIRS.values()]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from eigen_zeth_amd.stark.build_airs import build_all as _b
    print("\n".join(_b("--force" in sys.argv)))
