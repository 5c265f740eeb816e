"""eigen_zeth_amd/csrc/witness_host.hip (zp_stark_check_witness with ctx = NULL) with csrc/verify.hip's blob validation under AddressSanitizer +
UBSan on the host: a stand-alone program (tests/native/witness_check_fuzz.cpp) built from the two translation units as plain C++.  A valid case
must give the recorded report -- the checker's own (tests/witness_cases.py) -- and a few thousand seeded mutations of blob, public inputs, trace,
trace length and logn must be judged or refused without a finding.  Nothing is preloaded; nothing runs on a GPU."""
import os
import subprocess

import numpy as np

import witness_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_file(path, blob, trace, pubs, logn, chal):
    rep, counts, first = WC.oracle_report(blob, trace, pubs, logn, chal)
    u = lambda v: np.array([int(x) for x in v], dtype=np.uint64)
    np.concatenate([u([blob.size]), blob, u([len(pubs)]), u(pubs), u([logn, int(chal is not None)]), u(chal or [0, 0, 0]),
                    np.ascontiguousarray(trace, dtype=np.uint64).reshape(-1), u(rep), u(counts), u(first)]).tofile(path)
    return rep


def test_witness_check_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17"]
    csrc = os.path.join(ROOT, "eigen_zeth_amd", "csrc")
    objs = []
    for unit in ("witness_host", "verify"):
        objs.append(str(tmp_path / (unit + ".o")))
        subprocess.check_call(["g++", *san, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", os.path.join(csrc, unit + ".hip"), "-o", objs[-1]])
    exe = str(tmp_path / "witness_check_fuzz")
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "native", "witness_check_fuzz.cpp"), *objs, "-o", exe, "-lpthread"])
    # a stage-2 statement with one cell flipped (explicit challenge), a satisfied one (derived challenge), and a random program with eight sparse columns
    _, blob, trace, pubs = WC.honest_case("chunk16", 4)
    cases = [("flipped", blob, WC.flipped(trace, 3, 7), pubs, 4, WC.EXPLICIT_CHALLENGE, WC.VIOLATED), ("honest", blob, trace, pubs, 4, None, WC.SATISFIED)]
    pblob, ptrace, ppubs, _ = WC.random_case("periods", 4)
    cases.append(("periods", pblob, ptrace, ppubs, 4, None, WC.VIOLATED))
    for name, b, t, pb, logn, chal, verdict in cases:
        path = str(tmp_path / (name + ".bin"))
        assert case_file(path, b, t, pb, logn, chal)[0] == verdict
        out = subprocess.run([exe, path, "1200"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("ok:"), out.stdout
