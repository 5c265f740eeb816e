"""The aggregated-proof verifier of eigen_zeth_amd/csrc/verify.hip (zp_aggregate_verify, ctx = NULL) under AddressSanitizer + UBSan on the host:
a stand-alone program (tests/native/agg_verify_fuzz.cpp, its own main; nothing is loaded into Python) links verify.hip compiled as plain C++ and
feeds it one good level-2 text and hundreds of seeded byte- and token-level mutations of it with ZP_VERIFY_HEADER_ONLY.  Every call must end in a
verdict (ZP_OK) and no sanitizer may fire: the text sizes the sponge streams, the index tables and the batch of fixed-column evaluations."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aggregate_verifier_under_sanitizers(tmp_path, tables):
    from eigen_zeth_amd.stark import agg_statements as AS
    from test_aggregate_verify_native import get_world
    w = get_world(tables)
    table, text = str(tmp_path / "statements.bin"), str(tmp_path / "level2.json")
    AS.write_table(table, w.statements)
    with open(text, "w") as f:
        f.write(json.dumps(w.top, separators=(",", ":")))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17"]
    obj, exe = str(tmp_path / "verify.o"), str(tmp_path / "agg_verify_fuzz")
    subprocess.check_call(["g++", *san, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c",
                           os.path.join(ROOT, "eigen_zeth_amd", "csrc", "verify.hip"), "-o", obj])
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "native", "agg_verify_fuzz.cpp"), obj, "-o", exe, "-lpthread"])
    out = subprocess.run([exe, table, text, "400"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:"), out.stdout
    counts = dict(kv.split(":") for kv in out.stdout.split("verdicts")[1].split())
    assert int(counts["1"]) > 0 and int(counts["9"]) > 0, out.stdout      # the mutations reach past the grammar
