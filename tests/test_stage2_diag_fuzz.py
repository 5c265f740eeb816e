"""eigen_zeth_amd/csrc/stage2_diag_host.hip (zp_stark_diagnose_stage2 with ctx = NULL) under AddressSanitizer + UBSan on the host: a stand-alone
program (tests/native/stage2_diag_fuzz.cpp) built from the translation unit as plain C++.  A valid case must give the recorded records -- the
multiset comparison of tests/stage2_diag_cases.py -- and a few thousand seeded mutations of blob, trace, trace length, logn and n_stage2, with cut
blobs and short or odd traces, must be judged or refused (ZP_OK or ZP_ERR_ARG, nothing else) without a finding.  Nothing is preloaded; nothing runs on a GPU."""
import os
import subprocess

import numpy as np

import stage2_diag_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_file(path, blob, trace, logn):
    u = lambda v: np.array([int(x) for x in v], dtype=np.uint64)
    want = SC.expected(blob, trace, logn)
    np.concatenate([u([blob.size]), blob, u([logn]), np.ascontiguousarray(trace, dtype=np.uint64).reshape(-1), u(sum(want, []))]).tofile(path)
    return want


def test_stage2_diagnosis_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17"]
    obj, exe = str(tmp_path / "stage2_diag_host.o"), str(tmp_path / "stage2_diag_fuzz")
    subprocess.check_call(["g++", *san, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c",
                           os.path.join(ROOT, "eigen_zeth_amd", "csrc", "stage2_diag_host.hip"), "-o", obj])
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "native", "stage2_diag_fuzz.cpp"), obj, "-o", exe, "-lpthread"])
    # a lookup broken at one row, an honest trace and a permutation over colliding values; 2^12 rows also take the path that shares the values out over threads
    for name, logn, verdicts in (("broken_lookup", 5, [SC.HOLDS, SC.FAILS]), ("honest_chunk16", 4, [SC.HOLDS, SC.HOLDS]), ("collide:hi32:broken", 12, [SC.FAILS])):
        blob, trace, _ = SC.case(name, logn)
        path = str(tmp_path / (name.replace(":", "_") + ".bin"))
        assert [r[0] for r in case_file(path, blob, trace, logn)] == verdicts
        out = subprocess.run([exe, path, "1200" if logn < 12 else "150"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("ok:"), out.stdout
