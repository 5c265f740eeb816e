"""LDS slot addresses of the NTT pass kernels on the host, exhaustively (tests/native/ntt_slots_check.cpp over csrc/ntt_geo.hpp).

The kernels compute a slot's LDS byte offset as (lane part) ^ (uniform bits of k_j inside the column field) + (uniform slot bits of
k_j) -- one instruction per write -- and the copy-out read as (lane part) ^ constant.  The program walks every shape dispatch_pass
builds, every round, every odd j0inv, every lane and every register, compares with lpos(slot_of(...), t) / lpos(sigma_of_k(k), t2)
and checks that a round's writes and the copy-out's reads are permutations of the tile.  Built plain and under
-fsanitize=address,undefined; it stands alone, nothing is preloaded and nothing runs on a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eigen_zeth_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ntt_slots_check.cpp")


def dispatch_shapes():
    """(A1, A2, A3, LOGT) of every case of dispatch_pass, the 64-bit-offset forms folded onto their geometry"""
    with open(os.path.join(CSRC, "ntt.hip")) as f:
        text = f.read()
    body = text[text.index("int32_t dispatch_pass("):]
    body = body[:body.index("#undef ZP_PASS_SHAPE")]
    found = re.findall(r"ZP_PASS_SHAPE\((\d), (\d), (\d), (\d), (?:true|false)\);", body)
    assert len(found) >= 11, found
    return sorted({tuple(int(v) for v in s) for s in found})


@pytest.mark.parametrize("flags", [["-O2"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]], ids=["plain", "sanitizers"])
def test_every_slot_address(tmp_path, flags):
    exe = str(tmp_path / "ntt_slots_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[-1].startswith("ok: "), out.stdout
    rows = [tuple(int(v) for v in l.split()[1:5]) + (int(l.split()[6]), int(l.split()[8]), int(l.split()[10])) for l in lines[:-1]]
    # every shape of dispatch_pass, and no other
    assert sorted(r[:4] for r in rows) == dispatch_shapes(), rows
    total = 0
    for a1, a2, a3, logt, factored, copy_out, cases in rows:
        # the kernels take the factored form wherever lpos has no slot swizzle; the table copy-out runs on two-round shapes
        assert factored == (0 if (logt < 4 and a3 > 0) else 1), (a1, a2, a3, logt)
        assert copy_out or a3 > 0, (a1, a2, a3, logt)
        # nothing sampled: per round 8 values of j0inv x all R T elements of the tile, and R T copy-out reads
        tile = (1 << (a1 + a2 + a3)) << logt
        rounds = 2 + (1 if a3 > 0 else 0)
        assert cases == 8 * tile * rounds + (tile if copy_out else 0), (a1, a2, a3, logt, cases)
        total += cases
    assert int(lines[-1].split()[1]) == total
