"""csrc/witness_merge.hpp -- the merge of per-rank constraint-check results into one report, the only host-only logic of the witness check over the
ranks -- as a stand-alone program under the host sanitizers (tests/native/witness_merge_check.cpp: all ranks empty, one rank violated, ties on the
first row).  Nothing is preloaded; nothing runs on a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "witness_merge_check")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "native", "witness_merge_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr
