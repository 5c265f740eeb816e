"""Every proof / public-input vector the reference holds (tests/golden/ref_proofs.json, made by tests/golden/extract_ref_proofs.py), run
through the mirror of the reference's consumer (eigen_zeth_amd/service/consumer.py = src/settlement/ethereum/mod.rs:445-481):

* the reference's ONLY result-pinning test on proof data, `test_parse_proof` (mod.rs:487-571): same input, the same eight U256, in the same
  order; `test_parse_public_input` (mod.rs:573-589) likewise;
* all three reference-held proofs (mod.rs:489-512; worker.rs:760-761 = custom/methods.rs:710-711; proof/proof.json) parse, lie on the
  curve / the twist in JSON order, have public inputs below r -- and NONE of them verifies under the key in contracts/EigenZkVM.json for
  any assignment of roles (tests/golden/ref_vk.json): they pin the FORMAT the settlement layer accepts, not arithmetic;
* the mirror's error behaviour on what the reference's `as_str().ok_or(..)?` / `from_dec_str(..)?` reject."""
import itertools
import json
import os

import pytest

from eigen_zeth_amd.service import consumer as CS
from oracle import bn254_pairing as BP
from oracle import naive_bn254 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ref_proofs.json")) as f:
        return json.load(f)


def _lines(spec):
    """text whose line k (1-based) is spec[k]; lines not in spec are empty"""
    return "\n".join(spec.get(k, "") for k in range(1, max(spec) + 2))


def _rust_str(obj):
    return json.dumps(obj).replace("\\", "\\\\").replace('"', '\\"')


def test_fixture_is_what_the_extractor_produces(fx, tmp_path):
    """the committed fixture is exactly what the extractor writes for a source tree that holds the fixture's vectors where the fixture
    says they are (file, line span, test function, literal form): every vector, expected output, field order and source location
    round-trips through the extractor's parsing"""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("extract_ref_proofs", os.path.join(ROOT, "tests", "golden", "extract_ref_proofs.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    span = lambda s, pat: [int(v) for v in re.search(pat, s).groups()]
    p0, p1, p2, p3 = fx["proofs"][0], fx["public_inputs"][0], fx["proofs"][1], fx["proofs"][2]
    i0, i1, a0, a1 = span(p0["source"], r"mod\.rs:(\d+)-(\d+) \(input\), :(\d+)-(\d+)")
    u0, u1 = span(p1["source"], r"mod\.rs:(\d+)-(\d+)")
    mod = {i0 - 1: "fn test_parse_proof() {", i0: 'let input = r#"' + json.dumps(p0["proof"]), i1: '"#;', a1 + 3: "fn test_parse_public_input() {",
           u1 + 3: "fn test_from_conf_path() {"}
    for k, (name, val) in enumerate(zip(p0["expected_fields_in_order"], p0["expected_u256_in_order"])):
        mod[a0 + k] = 'assert_eq!(proof.%s, U256::from_dec_str("%s").unwrap());' % (name, val)
    mod[u0 + 2] = 'let input = r#"' + json.dumps(p1["public_input"]) + '"#;'
    mod[u0 + 3] = 'assert_eq!(input[0], U256::from_dec_str("%s").unwrap());' % p1["expected_u256"]
    w0, c0 = span(p2["source"], r"worker\.rs:(\d+)-\d+ = src/settlement/custom/methods\.rs:(\d+)-")
    worker = {w0: 'public_input: "%s".to_string(),' % _rust_str(p2["public_input"]), w0 + 1: 'proof: "%s".to_string(),' % _rust_str(p2["proof"])}
    methods = {c0: '"%s".to_string(),' % _rust_str(p2["proof"]), c0 + 1: '"%s".to_string(),' % _rust_str(p2["public_input"])}
    ref = tmp_path / "ref"
    for rel, text in (("src/settlement/ethereum/mod.rs", _lines(mod)), ("src/settlement/worker.rs", _lines(worker)),
                      ("src/settlement/custom/methods.rs", _lines(methods)), ("proof/proof.json", json.dumps(p3["proof"])),
                      ("proof/public_input.json", json.dumps(p3["public_input"]))):
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    ex.REF = str(ref)
    ex.OUT = str(tmp_path / "again.json")
    ex.main()
    assert json.load(open(ex.OUT)) == fx


def test_reference_test_parse_proof_vector(fx):
    """mod.rs:487-571: parse_proof(input) == the asserted tuple, field by field, in the reference's order"""
    f = fx["proofs"][0]
    assert f["pinned_by_reference_test"] == "test_parse_proof"
    assert f["expected_fields_in_order"] == ["a.x", "a.y", "b.x[0]", "b.x[1]", "b.y[0]", "b.y[1]", "c.x", "c.y"]
    pr = CS.parse_proof(json.dumps(f["proof"]))
    assert pr.as_u256_tuple() == tuple(int(v) for v in f["expected_u256_in_order"])
    got = {"a.x": pr.a.x, "a.y": pr.a.y, "b.x[0]": pr.b.x[0], "b.x[1]": pr.b.x[1], "b.y[0]": pr.b.y[0], "b.y[1]": pr.b.y[1], "c.x": pr.c.x,
           "c.y": pr.c.y}
    for name, want in zip(f["expected_fields_in_order"], f["expected_u256_in_order"]):
        assert got[name] == int(want), name
    # whitespace and key order of the text do not matter, extra keys are ignored (the vector carries "protocol" and "curve")
    assert CS.parse_proof(json.dumps(f["proof"], indent=8, sort_keys=True)) == pr and "protocol" in f["proof"] and "curve" in f["proof"]


def test_reference_test_parse_public_input_vector(fx):
    f = fx["public_inputs"][0]
    assert CS.parse_public_input(json.dumps(f["public_input"], indent=2)) == [int(f["expected_u256"])]


def test_every_reference_held_proof_parses_and_is_well_formed(fx):
    assert len(fx["proofs"]) == 3
    for f in fx["proofs"]:
        pr = CS.parse_proof(json.dumps(f["proof"]))
        assert B.on_curve(tuple(pr.a)) and B.on_curve(tuple(pr.c)), f["source"]
        assert B.on_curve_g2((pr.b.x, pr.b.y)), f["source"]                                    # JSON order = (c0, c1): nothing swapped
        assert not B.on_curve_g2(((pr.b.x[1], pr.b.x[0]), (pr.b.y[1], pr.b.y[0]))), f["source"]
        if "public_input" in f:
            assert CS.parse_public_input(json.dumps(f["public_input"]))[0] < B.R
    # the stand-in files are what tests/golden/ref_proof.json holds (round 1's fixture)
    assert fx["proofs"][2]["proof"] == json.load(open(os.path.join(ROOT, "tests", "golden", "ref_proof.json")))
    assert fx["proofs"][2]["public_input"] == json.load(open(os.path.join(ROOT, "tests", "golden", "ref_public_input.json")))


def _vk():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_vk.json")))
    g1 = [tuple(int(v) for v in p) for p in d["g1"]]
    g2 = [((int(w[0]), int(w[1])), (int(w[2]), int(w[3]))) for w in d["g2_words"]]
    return g1, g2


@pytest.mark.parametrize("which", [0, 1])
def test_no_reference_held_proof_verifies_under_the_reference_key(fx, which):
    """Groth16: e(A, B) = e(alpha, beta) e(IC0 + pub IC1, gamma) e(C, delta), all 6 x 6 role assignments of the pushed points (the
    third fixture, proof/proof.json, is covered by tests/test_ref_vk.py).  mod.rs:489-512 comes without a public input of its own: it
    is tried with the public input of the neighbouring test AND with the two other reference-held public inputs."""
    g1, g2 = _vk()
    f = fx["proofs"][which]
    pr = CS.parse_proof(json.dumps(f["proof"]))
    pubs = [int(f["public_input"][0])] if "public_input" in f else \
        [int(fx["public_inputs"][0]["expected_u256"])] + [int(g["public_input"][0]) for g in fx["proofs"] if "public_input" in g]
    neg = lambda p: (p[0], (-p[1]) % B.Q)
    A, Bp, Cp = tuple(pr.a), (pr.b.x, pr.b.y), tuple(pr.c)
    m_ab = BP.miller(Bp, A)
    m_alpha = {(i, j): BP.miller(g2[j], neg(g1[i])) for i in range(3) for j in range(3)}
    m_c = {j: BP.miller(g2[j], neg(Cp)) for j in range(3)}
    for pub in pubs:
        m_x = {}
        for i0, i1 in itertools.permutations(range(3), 2):
            vkx = B.add(g1[i0], B.mul(g1[i1], pub))
            for j in range(3):
                m_x[(i0, i1, j)] = BP.miller(g2[j], neg(vkx))
        for (ia, i0, i1) in itertools.permutations(range(3), 3):
            for (jb, jg, jd) in itertools.permutations(range(3), 3):
                f12 = BP.f_mul(BP.f_mul(m_ab, m_alpha[(ia, jb)]), BP.f_mul(m_x[(i0, i1, jg)], m_c[jd]))
                assert BP.final_exp(f12) != BP.ONE, (f["source"], pub, ia, i0, i1, jb, jg, jd)


def test_error_behaviour_of_the_mirror(fx):
    good = fx["proofs"][0]["proof"]

    def broken(mut):
        v = json.loads(json.dumps(good))
        mut(v)
        return json.dumps(v)
    with pytest.raises(CS.ParseError):
        CS.parse_proof("not json")
    with pytest.raises(CS.ParseError):                      # a number instead of a string: as_str() is None -> "invalid json data"
        CS.parse_proof(broken(lambda v: v["pi_a"].__setitem__("x", 5)))
    with pytest.raises(CS.ParseError):                      # a missing coordinate indexes to Null
        CS.parse_proof(broken(lambda v: v["pi_b"]["y"].pop()))
    with pytest.raises(CS.ParseError):                      # hex is not decimal
        CS.parse_proof(broken(lambda v: v["pi_c"].__setitem__("y", "0x10")))
    with pytest.raises(CS.ParseError):                      # 2^256 overflows U256
        CS.parse_proof(broken(lambda v: v["pi_c"].__setitem__("x", str(1 << 256))))
    assert CS.parse_proof(broken(lambda v: v["pi_c"].__setitem__("x", str((1 << 256) - 1)))).c.x == (1 << 256) - 1
    with pytest.raises(CS.ParseError):
        CS.parse_public_input("[]")
    with pytest.raises(CS.ParseError):
        CS.parse_public_input("[12]")
    assert CS.parse_public_input('["12", "ignored"]') == [12]


def test_proof_result_record_shape(fx):
    """src/db/mod.rs:63-71 through serde_json: roots are arrays of 32 numbers; the strings are stored verbatim"""
    f = fx["proofs"][1]
    js = CS.proof_result_json(1, json.dumps(f["proof"]), json.dumps(f["public_input"]), bytes(32), bytes(range(32)))
    d = json.loads(js)
    assert list(d) == ["block_number", "proof", "public_input", "pre_state_root", "post_state_root"]
    assert d["pre_state_root"] == [0] * 32 and d["post_state_root"] == list(range(32))
    assert CS.parse_proof(d["proof"]) == CS.parse_proof(json.dumps(f["proof"]))
    with pytest.raises(ValueError):
        CS.proof_result_json(1, "", "", bytes(31), bytes(32))
