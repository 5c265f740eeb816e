"""zp_stark_verify_bn128 / zp_stark_verify_batch_bn128 with ctx = NULL: the whole BN128-hash-mode verifier on the host (no GPU needed) against the
CPU checker (oracle/stark_verify.py, expect["hash"] == "bn128") check for check -- honest proofs of every shape, single-field mutations by verdict
class, seeded random mutations by accept / reject, a batch, and the host-only translation units under AddressSanitizer + UBSan (a stand-alone
program, run as a subprocess)."""
import os
import subprocess

import numpy as np
import pytest

import stark_verify_bn128_cases as BC
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
from eigen_zeth_amd.stark import prover as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bn_tables():
    return bn254_poseidon_params(17)


@pytest.fixture(scope="module")
def cases(tables, bn_tables):
    cpu = BC.cpu_backend(tables, bn_tables)
    out = {name: BC.make_case(name, cpu) for name in BC.SHAPES}
    out["vair"] = BC.make_vair_case(cpu, tables)
    return out


def verify(case, text, bn_tables, flags=0):
    return native.stark_verify_bn128(case.program, text, case.params, flags, bn_tables=bn_tables)


@pytest.mark.parametrize("name", BC.NAMES)
def test_honest_proofs_are_accepted_with_the_checkers_indices(cases, tables, bn_tables, name):
    case = cases[name]
    assert BC.oracle_class(case, case.proof, tables, bn_tables) == native.VERDICT_ACCEPT
    verdict, where, indices = verify(case, case.text, bn_tables)
    assert (verdict, where) == (native.VERDICT_ACCEPT, -1)
    assert indices == BC.oracle_indices(case, tables, bn_tables)
    for flags in (native.VERIFY_HEADER_ONLY, native.VERIFY_TRUST_OPENINGS):
        assert verify(case, case.text, bn_tables, flags) == (native.VERDICT_ACCEPT, -1, indices)
    if name == "vair":         # 47 columns; the 16-ary commitment of the public inputs
        assert len(case.proof["publics"]) > 64 and int(case.program[1]) + int(case.program[2]) == 47
    if name == "wide64":       # a two-block leaf sponge, ungrouped; 48-value FRI leaves
        assert len(case.proof["queries"][0]["trace"]["values"]) == 64 and len(case.proof["queries"][0]["fri"][0]["values"]) == 48


@pytest.mark.parametrize("name", BC.NAMES)
def test_single_field_mutations_get_the_checkers_class(cases, tables, bn_tables, name):
    case = cases[name]
    seen = {}
    for label, flags, m in BC.single_field_mutations(case):
        want = BC.oracle_class(case, m, tables, bn_tables, flags)
        verdict, where, _ = verify(case, PR.proof_to_json(m), bn_tables, flags)
        assert verdict == want, (name, label, verdict, want)
        assert (where >= 0) == (verdict in (native.VERDICT_OPENING, native.VERDICT_FRI)), (name, label, where)
        seen[label] = verdict
    # the classes these mutations are known to give (measured with the checker alone)
    trees = [t[0] for t in BC.tree_shapes(case)]
    for tree in trees:
        assert seen[tree + " value"] == seen[tree + " last value"] == native.VERDICT_OPENING, tree
        for word in ("sibling word", "own-slot word", "top-level word", "path word = r", "zero slot := 1"):
            assert seen.get(tree + " " + word, native.VERDICT_OPENING) == native.VERDICT_OPENING, (tree, word)
    assert any(t + " zero slot := 1" in seen for t in trees) or name in ("fib", "perm", "chunk16")
    assert seen["trace root"] == seen["quotient root"] == seen["evaluation at zeta"] == seen["public input"] == native.VERDICT_IDENTITY
    assert seen["fri root"] == seen["final-layer word"] == seen["index ^ 1"] == seen["queries shortened"] == native.VERDICT_INDICES
    assert seen["final-layer word, header only"] == native.VERDICT_FINAL_DEGREE
    assert seen["trace root = r"] == seen["fri root = r"] == native.VERDICT_MALFORMED
    assert seen["params.logb"] == seen["params.pow_bits"] == seen["hash relabelled gl"] == seen["root32"] == native.VERDICT_PARAMS
    assert seen["trace value of the queried row, trusted openings"] == seen["last-layer FRI value, trusted openings"] == native.VERDICT_FRI
    assert seen.get("trace value of another row, trusted openings", 0) == native.VERDICT_ACCEPT      # a grouped leaf: only the queried row is read
    assert ("trace value of another row, trusted openings" in seen) == (BC.tree_shapes(case)[0][3] > 0) and (name != "fib" or BC.tree_shapes(case)[0][3] == 3)
    assert seen["trace path word, trusted openings"] == native.VERDICT_ACCEPT
    if "stage2" in case.proof["roots"]:
        assert seen["stage2 opening dropped"] == seen["stage2 root dropped"] == native.VERDICT_MALFORMED


@pytest.mark.parametrize("name", BC.NAMES)
def test_seeded_random_mutations_accept_and_reject_like_the_checker(cases, tables, bn_tables, name):
    case = cases[name]
    accepted = 0
    for path, new, m in BC.random_mutations(case, 100, 200, 0x5EED + len(name)):
        want = BC.oracle_class(case, m, tables, bn_tables) == native.VERDICT_ACCEPT
        got = verify(case, PR.proof_to_json(m), bn_tables)[0] == native.VERDICT_ACCEPT
        assert got == want, (name, path, new, BC.get(case.proof, path))
        accepted += want
    assert accepted < 30          # a mutation is accepted only where it names the same field element (p for 0)


def test_batch_verdicts_are_the_single_call_verdicts(tables, bn_tables):
    cpu = BC.cpu_backend(tables, bn_tables)
    cs = [BC.make_case("chunk16", cpu, seed) for seed in (21, 22, 23, 24, 25)]
    texts = [c.text for c in cs]
    texts[1] = PR.proof_to_json(BC.mutated(cs[1].proof, ("queries", 3, "fri", 1, "values", 5), BC.bump))
    texts[3] = PR.proof_to_json(BC.mutated(cs[3].proof, ("evals", "zw", 2, 0), BC.bump))
    a, b = (verify(cs[0], texts[i], bn_tables)[0] for i in (1, 3))
    assert (a, b) == (native.VERDICT_OPENING, native.VERDICT_IDENTITY)
    assert native.stark_verify_batch_bn128(cs[0].program, texts, cs[0].params, bn_tables=bn_tables) == [0, a, 0, b, 0]
    assert native.stark_verify_batch_bn128(cs[0].program, texts, cs[0].params, threads=3, bn_tables=bn_tables) == [0, a, 0, b, 0]


def test_the_grammar_of_field_elements_and_the_callers_mistakes(cases, bn_tables):
    case = cases["fib"]
    word = case.proof["queries"][0]["trace"]["path"][0][3]
    root = case.proof["roots"]["trace"][0]
    swap = lambda old, new: case.text.replace('"%s"' % old, new, 1)
    assert verify(case, swap(word, '"0%s"' % word), bn_tables)[0] == native.VERDICT_MALFORMED         # a leading zero
    assert verify(case, swap(word, '"+%s"' % word), bn_tables)[0] == native.VERDICT_MALFORMED         # a sign
    assert verify(case, swap(word, '""'), bn_tables)[0] == native.VERDICT_MALFORMED                   # no digit
    assert verify(case, swap(word, word), bn_tables)[0] == native.VERDICT_MALFORMED                   # not quoted
    assert verify(case, swap(word, '"%s"' % ("9" * 5000)), bn_tables)[0] == native.VERDICT_OPENING    # any length: >= r, equal to nothing
    assert verify(case, swap(root, '"%s"' % ("9" * 5000)), bn_tables)[0] == native.VERDICT_MALFORMED  # a root >= r
    assert verify(case, swap(root, '"%s","0"' % root), bn_tables)[0] == native.VERDICT_MALFORMED      # a root of two elements
    assert verify(case, case.text + " ", bn_tables)[0] == native.VERDICT_ACCEPT
    assert verify(case, case.text[:-1], bn_tables)[0] == native.VERDICT_MALFORMED
    with pytest.raises(native.ZpError):                              # a program blob that does not parse
        native.stark_verify_bn128(case.program[:-1], case.text, case.params, bn_tables=bn_tables)
    with pytest.raises(native.ZpError):                              # a table entry that is not reduced mod r
        rc, mds, rp = bn_tables
        native.stark_verify_bn128(case.program, case.text, case.params, bn_tables=([BC.R] + list(rc[1:]), mds, rp))
    lib = native.load_library()
    v, w = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    p32 = lambda a: a.ctypes.data_as(native.C.POINTER(native.C.c_int32))
    raw = case.text.encode()
    prog = case.program
    args = (prog.ctypes.data_as(native._u64p), prog.size, raw, len(raw), *BC.SHAPES["fib"])
    assert lib.zp_stark_verify_bn128(None, *args, 0, None, None, 0, 0, p32(v), p32(w), None) == -1      # ctx = NULL without tables
    # the Goldilocks-mode call does not read the text: its roots are not that grammar's
    assert native.stark_verify(case.program, case.text, dict(case.params.to_dict(), hash="gl"))[0] == native.VERDICT_MALFORMED


def test_verifier_under_sanitizers(tmp_path, cases, bn_tables):
    """csrc/verify.hip + csrc/proofparse.hip as plain C++ under ASan + UBSan, linked with nothing else: one valid BN128-mode case, then 1000 seeded
    byte and digit mutations of the text through zp_stark_verify_bn128(NULL, ...): every one ends in a verdict or an error code"""
    case = cases["fib"]
    prog, text, tab = str(tmp_path / "program.bin"), str(tmp_path / "proof.json"), str(tmp_path / "tables.bin")
    case.program.tofile(prog)
    open(text, "w").write(case.text)
    rc, mds, rp = bn_tables
    np.concatenate([native.Prover._fr_words(rc).reshape(-1), native.Prover._fr_words([v for row in mds for v in row]).reshape(-1)]).tofile(tab)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O2", "-std=c++17"]      # (-O2: a width-17 permutation under UBSan is ~10 ms)
    objs = []
    for unit in ("verify", "proofparse"):
        objs.append(str(tmp_path / (unit + ".o")))
        subprocess.check_call(["g++", *san, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c",
                               os.path.join(ROOT, "eigen_zeth_amd", "csrc", unit + ".hip"), "-o", objs[-1]])
    exe = str(tmp_path / "stark_verify_bn128_fuzz")
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "native", "stark_verify_bn128_fuzz.cpp"), *objs, "-o", exe, "-lpthread"])
    out = subprocess.run([exe, prog, text, tab, str(rp), *[str(v) for v in BC.SHAPES["fib"]], "1000"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:"), out.stdout
