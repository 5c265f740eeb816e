"""zp_stark_verify / zp_stark_verify_batch / zp_merkle_verify_batch through a ctx on the MI355X: the opening kernels (one lane per opening, and
the 12-lane walk below `verify_lane_min`) against the CPU checker's Merkle verifier, whole proofs made by zp_stark_prove against the checker's
verdict classes and against the host-only path, and the compiled host host/verify_chunk on what host/prove_chunk wrote."""
import json
import os
import subprocess

import numpy as np
import pytest

import stark_verify_cases as SC
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR, prover as PR, verifier_air as VA
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE, WALK = 1, 1 << 30                    # verify_lane_min: every call on the lane kernel / on the walk kernel


@pytest.fixture
def form(prover, request):
    prover.set_tuning("verify_lane_min", request.param)
    yield request.param
    prover.set_tuning("verify_lane_min", 0)


_OPENINGS = {}


def tree_openings(prover, rc, mds, width, depth, n, seed):
    """a tree from zp_merkle_commit, n openings of it with every 7th corrupted (value, sibling, index in turn), and the checker's flags (made once,
    shared by the two kernel forms)"""
    key = (width, depth, n, seed, rc.tobytes()[:64])
    if key not in _OPENINGS:
        _OPENINGS[key] = _tree_openings(prover, rc, mds, width, depth, n, seed)
    return _OPENINGS[key]


def _tree_openings(prover, rc, mds, width, depth, n, seed):
    M = 1 << depth
    cols = O.random_field((width, M), seed)
    cols[0, 0] = 0
    d_cols, d_tree = prover.upload(cols), prover.alloc((2 * M - 1) * 4)
    prover.merkle_commit(d_cols, M, width, d_tree)
    tree = prover.download(d_tree, (2 * M - 1, 4))
    assert (tree == O.merkle_commit(cols, rc, mds)).all()
    rng = np.random.default_rng(seed)
    index = rng.integers(0, M, size=n, dtype=np.uint64)
    index[0] = 0
    values = np.ascontiguousarray(cols[:, index.astype(np.int64)].T)
    paths = np.zeros((n, depth, 4), dtype=np.uint64)
    for o in range(n):
        paths[o] = O.merkle_path(tree, int(index[o]))
    for k, o in enumerate(range(3, n, 7)):
        if k % 3 == 0:
            values[o, (o * 5) % width] = (int(values[o, (o * 5) % width]) + 1) % O.P
        elif k % 3 == 1 and depth:
            paths[o, o % depth, o % 4] = (int(paths[o, o % depth, o % 4]) + 1) % O.P
        elif depth:
            index[o] ^= np.uint64(1 << (o % depth))
        else:
            values[o, 0] = (int(values[o, 0]) + 1) % O.P
    want = np.array([O.merkle_verify(O.linear_hash(values[o], rc, mds), M, int(index[o]), paths[o], tree[-1], rc, mds) for o in range(n)], dtype=np.uint8)
    return values, index, paths, tree[-1], want


@pytest.mark.parametrize("form", [LANE, WALK], indirect=True)
@pytest.mark.parametrize("depth", [0, 1, 5, 12])
def test_merkle_verify_batch_matches_the_checker(prover, tables, form, depth):
    rc, mds = tables
    for width in (1, 3, 4, 5, 8, 9, 16, 17, 76):
        for n in (1, 63, 64, 65, 1000):
            values, index, paths, root, want = tree_openings(prover, rc, mds, width, depth, n, 7000 + 100 * depth + width)
            got = prover.merkle_verify_batch(values, index, paths, root)
            assert (got == want).all(), (width, depth, n, np.flatnonzero(got != want)[:8])
            assert n < 8 or (0 < int(want.sum()) < n)          # both outcomes are in the batch


@pytest.mark.parametrize("form", [LANE, WALK], indirect=True)
def test_merkle_verify_batch_injected_tables(prover, tables, form):
    """a non-default matrix and constants through zp_set_constants: the kernels' general-matrix path"""
    rc2 = O.random_field((360,), 29)
    mds2 = (O.random_field((144,), 30) % np.uint64(1 << 20)).astype(np.uint64)
    try:
        prover.set_constants(native.ZP_CONST_POSEIDON_RC, rc2)
        prover.set_constants(native.ZP_CONST_POSEIDON_MDS, mds2)
        for width, depth, n in ((3, 5, 65), (17, 5, 130), (76, 12, 65)):
            values, index, paths, root, want = tree_openings(prover, rc2, mds2, width, depth, n, 7700 + width)
            assert (prover.merkle_verify_batch(values, index, paths, root) == want).all(), (width, depth, n)
    finally:
        prover.set_constants(native.ZP_CONST_POSEIDON_RC, tables[0])
        prover.set_constants(native.ZP_CONST_POSEIDON_MDS, tables[1])


def device_case(prover, name, seed=11):
    """the proof zp_stark_prove writes for a toy shape"""
    a = SC.SHAPES[name]
    air, tr, pub = SC.witness(name, a[0], seed)
    params = PR.StarkParams(*a[:5], pow_bits=a[5])
    d = prover.upload(tr)
    text = prover.stark_prove(air.name, air.program(), d, [int(v) for v in pub], *a)
    d.free()
    return SC.Case(name, air.program(), params, text)


def device_vair_case(prover, rc, mds):
    """SC.make_vair_case with both proofs made by zp_stark_prove: a verifier-AIR proof over one fib 2^5 proof (sparse periodic fixed columns, more than
    64 public inputs, a trace leaf of 47 values at blow-up 4); only the witness between the two proofs is assembled on the CPU"""
    from oracle.stark_cpu import CpuBackend
    air = AIR.get_air("fib")
    inner_shape = (5, 1, 2, 3, 3, 0)
    tr, pub = native.synth_trace(air.trace_kind, 5, air.width, 9)
    d = prover.upload(tr)
    inner = json.loads(prover.stark_prove(air.name, air.program(), d, [int(v) for v in pub], *inner_shape))
    d.free()
    shape = VA.Shape.of_proof(inner, 1)
    vair = VA.verifier_air(shape, rc, mds)
    wtrace, wpubs = VA.build_witness(shape, [inner], CpuBackend(rc, mds), air.digest_words())
    ap = VA.aggregation_params(shape, n_queries=4, fri_final_log=3)
    d = prover.upload(np.ascontiguousarray(wtrace))
    text = prover.stark_prove(vair.name, vair.program(), d, [int(v) for v in wpubs], ap.logn, ap.logb, ap.fri_logf, ap.fri_final_log, ap.n_queries, ap.pow_bits)
    d.free()
    return SC.Case("vair", vair.program(), ap, text)


@pytest.fixture(scope="module")
def cases(prover, tables):
    out = {name: device_case(prover, name) for name in SC.SHAPES}
    out["vair"] = device_vair_case(prover, *tables)
    return out


_CLASSES = {}


def checker_class(case, label, flags, m, rc, mds):
    """the CPU checker's class of a mutated proof: made once, shared by the two kernel forms"""
    key = (case.name, label, flags)
    if key not in _CLASSES:
        _CLASSES[key] = SC.oracle_class(case, m, rc, mds, flags)
    return _CLASSES[key]


@pytest.mark.parametrize("form", [LANE, WALK], indirect=True)
@pytest.mark.parametrize("name", list(SC.SHAPES) + ["vair"])
def test_device_proofs_verify_and_mutations_get_the_checkers_class(prover, tables, cases, form, name):
    rc, mds = tables
    case = cases[name]
    verdict, where, indices = native.stark_verify(case.program, case.text, case.params, prover=prover)
    assert (verdict, where) == (native.VERDICT_ACCEPT, -1) and indices == SC.oracle_indices(case, rc, mds)
    assert name != "vair" or len(case.proof["publics"]) > 64          # the digest path of the public inputs
    assert native.stark_verify(case.program, case.text, case.params) == (verdict, where, indices)
    for label, flags, m in SC.single_field_mutations(case):
        text = PR.proof_to_json(m)
        got = native.stark_verify(case.program, text, case.params, flags, prover=prover)
        assert got[0] == checker_class(case, label, flags, m, rc, mds), (name, label, got)
        assert got == native.stark_verify(case.program, text, case.params, flags), (name, label)


@pytest.mark.parametrize("form", [LANE, WALK], indirect=True)
def test_batch_verdicts_are_the_single_call_verdicts(prover, form):
    cs = [device_case(prover, "chunk16", seed) for seed in (21, 22, 23, 24, 25)]
    texts = [c.text for c in cs]
    q = ("queries", 3, "fri", 1)
    texts[1] = PR.proof_to_json(SC.mutated(cs[1].proof, q + ("values", 5), SC.bump))
    texts[3] = PR.proof_to_json(SC.mutated(cs[3].proof, ("evals", "zw", 2, 0), SC.bump))
    a, b = (native.stark_verify(cs[0].program, texts[i], cs[0].params, prover=prover)[0] for i in (1, 3))
    assert (a, b) == (native.VERDICT_OPENING, native.VERDICT_IDENTITY)
    assert native.stark_verify_batch(cs[0].program, texts, cs[0].params, prover=prover) == [0, a, 0, b, 0]
    assert native.stark_verify_batch(cs[0].program, texts, cs[0].params) == [0, a, 0, b, 0]


def test_compiled_host_verifies_what_the_compiled_prover_wrote(tmp_path):
    """host/verify_chunk (C++ on include/zeth_prover.h alone) accepts the proof host/prove_chunk wrote and rejects it with one digit changed inside "queries" (the
    lowest digit of an opened trace value: another field element, so the opening no longer hashes to the root)"""
    for exe in ("prove_chunk", "verify_chunk"):
        if not os.path.exists(os.path.join(ROOT, "host", exe)):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    air, tr, pub = SC.witness("chunk16", 10, 21)
    np.asarray(air.program(), dtype=np.uint64).tofile(tmp_path / "program.bin")
    np.ascontiguousarray(tr).tofile(tmp_path / "trace.bin")
    np.asarray(pub, dtype=np.uint64).tofile(tmp_path / "publics.bin")
    out, bad = tmp_path / "proof.json", tmp_path / "bad.json"
    shape = ["10", "1", "3", "3", "12", "6"]
    r = subprocess.run([os.path.join(ROOT, "host", "prove_chunk"), str(tmp_path / "program.bin"), str(tmp_path / "trace.bin"), str(tmp_path / "publics.bin"), *shape,
                        str(out), air.name], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    text = out.read_text()
    i = text.index('"values"', text.index('"queries"'))
    while not text[i].isdigit():
        i += 1
    while text[i + 1].isdigit():          # the LAST digit of the first opened value: another value below 2^64, whatever the first one was
        i += 1
    bad.write_text(text[:i] + ("1" if text[i] != "1" else "2") + text[i + 1:])
    verify = [os.path.join(ROOT, "host", "verify_chunk"), str(tmp_path / "program.bin")]
    r = subprocess.run(verify + [str(out), *shape], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("verdict 0 accept"), r.stdout + r.stderr
    r = subprocess.run(verify + [str(bad), *shape], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("verdict 7 opening"), r.stdout + r.stderr
