"""zp_stark_verify / zp_stark_verify_batch with ctx = NULL: the whole verifier on the host (no GPU needed), against the CPU checker
(oracle/stark_verify.py) check for check -- honest proofs of every toy shape, single-field mutations by verdict class, seeded random mutations by
accept / reject, a batch, and the host-only translation units under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import stark_verify_cases as SC
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import prover as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(SC.SHAPES) + ["vair"]


@pytest.fixture(scope="module")
def cpu(tables):
    from oracle.stark_cpu import CpuBackend
    return CpuBackend(*tables)


@pytest.fixture(scope="module")
def cases(cpu, tables):
    out = {name: SC.make_case(name, cpu) for name in SC.SHAPES}
    out["vair"] = SC.make_vair_case(cpu, *tables)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_honest_proofs_are_accepted_with_the_checkers_indices(cases, tables, name):
    case = cases[name]
    assert SC.oracle_class(case, case.proof, *tables) == native.VERDICT_ACCEPT
    verdict, where, indices = native.stark_verify(case.program, case.text, case.params)
    assert (verdict, where) == (native.VERDICT_ACCEPT, -1)
    assert indices == SC.oracle_indices(case, *tables)
    for flags in (native.VERIFY_HEADER_ONLY, native.VERIFY_TRUST_OPENINGS):
        assert native.stark_verify(case.program, case.text, case.params, flags) == (native.VERDICT_ACCEPT, -1, indices)
    assert len(case.proof["publics"]) > 64 or name != "vair"          # the digest path of the public inputs


@pytest.mark.parametrize("name", NAMES)
def test_single_field_mutations_get_the_checkers_class(cases, tables, name):
    case = cases[name]
    seen = {}
    for label, flags, m in SC.single_field_mutations(case):
        want = SC.oracle_class(case, m, *tables, flags)
        verdict, where, _ = native.stark_verify(case.program, PR.proof_to_json(m), case.params, flags)
        assert verdict == want, (name, label, verdict, want)
        assert (where >= 0) == (verdict in (native.VERDICT_OPENING, native.VERDICT_FRI)), (name, label, where)
        seen[label] = verdict
    # the table of the classes these mutations are known to give
    nq = len(case.proof["queries"])
    for tree in ["trace", "quotient"] + ["fri%d" % l for l in range(len(case.proof["fri"]["roots"]))] + (["stage2"] if "stage2" in case.proof["roots"] else []):
        assert seen[tree + " value"] == seen[tree + " path word"] == native.VERDICT_OPENING
    assert seen["index ^ 1"] == seen["queries shortened"] == native.VERDICT_INDICES
    assert seen["evaluation at zeta"] == seen["trace-root word"] == seen["public input"] == native.VERDICT_IDENTITY
    assert seen["params.logb"] == native.VERDICT_PARAMS
    assert seen["trace value, trusted openings"] == seen["last-layer FRI value, trusted openings"] == native.VERDICT_FRI
    if case.params.pow_bits:
        assert seen["pow_nonce + 1"] == seen["final-layer word"] == native.VERDICT_POW
    else:
        assert seen["final-layer word, header only"] == native.VERDICT_FINAL_DEGREE
    if "stage2" in case.proof["roots"]:
        assert seen["stage2 opening dropped"] == native.VERDICT_MALFORMED
    assert nq == case.params.n_queries


@pytest.mark.parametrize("name", NAMES)
def test_seeded_random_mutations_accept_and_reject_like_the_checker(cases, tables, name):
    case = cases[name]
    accepted = 0
    for path, new, m in SC.random_mutations(case, 300, 0x5EED + len(name)):
        want = SC.oracle_class(case, m, *tables) == native.VERDICT_ACCEPT
        got = native.stark_verify(case.program, PR.proof_to_json(m), case.params)[0] == native.VERDICT_ACCEPT
        assert got == want, (name, path, new, SC.get(case.proof, path))
        accepted += want
    assert accepted < 30          # a mutation is accepted only where it names the same field element (p for 0)


def test_batch_verdicts_are_the_single_call_verdicts(cpu):
    cs = [SC.make_case("chunk16", cpu, seed) for seed in (21, 22, 23, 24, 25)]
    texts = [c.text for c in cs]
    texts[1] = PR.proof_to_json(SC.mutated(cs[1].proof, ("queries", 3, "fri", 1, "values", 5), SC.bump))
    texts[3] = PR.proof_to_json(SC.mutated(cs[3].proof, ("evals", "zw", 2, 0), SC.bump))
    a, b = (native.stark_verify(cs[0].program, texts[i], cs[0].params)[0] for i in (1, 3))
    assert (a, b) == (native.VERDICT_OPENING, native.VERDICT_IDENTITY)
    assert native.stark_verify_batch(cs[0].program, texts, cs[0].params) == [0, a, 0, b, 0]
    assert native.stark_verify_batch(cs[0].program, texts, cs[0].params, threads=3) == [0, a, 0, b, 0]


def test_callers_mistakes_are_error_codes_not_verdicts(cases):
    case = cases["perm"]
    lib = native.load_library()
    with pytest.raises(native.ZpError):                              # a program blob that does not parse
        native.stark_verify(case.program[:-1], case.text, case.params)
    with pytest.raises(native.ZpError):                              # parameters outside the prover's ranges
        native.stark_verify(case.program, case.text, dict(case.params.to_dict(), fri_logf=9))
    bn = case.text.replace('"params":{', '"params":{"hash":"bn128",', 1)
    with pytest.raises(native.ZpError) as e:
        native.stark_verify(case.program, bn, case.params)
    assert e.value.code == -4                                        # ZP_ERR_UNSUPPORTED
    assert lib.zp_stark_verify(None, None, 0, b"", 0, 8, 1, 2, 3, 6, 4, 0, 0, None, None, None) == -1
    assert native.stark_verify(case.program, "", case.params)[0] == native.VERDICT_MALFORMED
    assert native.stark_verify(case.program, case.text[:-1], case.params)[0] == native.VERDICT_MALFORMED
    assert native.stark_verify(case.program, case.text + " ", case.params)[0] == native.VERDICT_ACCEPT


def test_verifier_under_sanitizers(tmp_path, cases):
    """csrc/verify.hip + csrc/proofparse.hip as plain C++ under ASan + UBSan: one valid case, then 1000 seeded byte and number mutations of the
    text through zp_stark_verify(NULL, ...): every one ends in a verdict or an error code"""
    case = cases["chunk16"]
    prog, text = str(tmp_path / "program.bin"), str(tmp_path / "proof.json")
    case.program.tofile(prog)
    open(text, "w").write(case.text)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17"]
    objs = []
    for unit in ("verify", "proofparse"):
        objs.append(str(tmp_path / (unit + ".o")))
        subprocess.check_call(["g++", *san, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c",
                               os.path.join(ROOT, "eigen_zeth_amd", "csrc", unit + ".hip"), "-o", objs[-1]])
    exe = str(tmp_path / "stark_verify_fuzz")
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "native", "stark_verify_fuzz.cpp"), *objs, "-o", exe, "-lpthread"])
    a = SC.SHAPES["chunk16"]
    out = subprocess.run([exe, prog, text, *[str(v) for v in a], "1000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:"), out.stdout
