"""The BN128-hash-mode verifier through a ctx: the device primitive zp_merkle16_verify_batch_bn254 (both job forms: 17 lanes per hash job below
`verify16_lane_min`, one lane per job from it on) against the CPU checker's 16-ary Merkle verifier; whole proofs made by zp_stark_prove_bn128
against the checker's classes and against the ctx = NULL call on the same texts; a batch; a ctx without the t = 17 tables."""
import subprocess
import sys

import numpy as np
import pytest

import stark_verify_bn128_cases as BC
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
from eigen_zeth_amd.stark import prover as PR
from oracle import oracle as O
from oracle import stark_verify as SV

pytestmark = pytest.mark.gpu
COOP, LANE = 1 << 30, 1                     # verify16_lane_min: every call on the 17-lanes-per-job kernel / on the lane-per-job kernel
R4 = [(SV.R_BN254 >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
# (leaves, leaf width): no level; one short group; one full group; a top group of 2 with 14 zero slots; 512 -> 32 -> 2 -> 1; a full tree.
# Widths on both sides of the 48-value packing and of the 56-value sponge block, up to three blocks
TREES = [(1, 3), (2, 47), (16, 48), (17, 1), (17, 113), (512, 49), (512, 56), (4096, 57), (4096, 112)]
COUNTS = [1, 2, 3, 4, 63, 64, 65, 1000]      # the 3-jobs-per-wave and 64-jobs-per-wave seams
_cache = {}


@pytest.fixture(scope="module")
def bn_tables():
    return bn254_poseidon_params(17)


@pytest.fixture(scope="module", params=[COOP, LANE], ids=["coop", "lane"])
def form(prover, request):
    prover.install_poseidon_bn254(17)
    prover.set_tuning("verify16_lane_min", request.param)
    yield request.param
    prover.set_tuning("verify16_lane_min", 0)


def fr_int(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


def openings_of(prover, bn_tables, M, W):
    """one committed tree and, per count, corrupted openings with the checker's flags -- made once, shared by both forms"""
    if (M, W) in _cache:
        return _cache[(M, W)]
    O.p254_set(17, bn_tables[2], bn_tables[0], bn_tables[1])
    rng = np.random.default_rng(1000 * M + W)
    cols = rng.integers(0, SV.P, size=(W, M), dtype=np.uint64)
    d_cols, d_tree = prover.upload(cols), prover.alloc(prover.merkle16_nodes(M) * 4)
    prover.merkle16_commit_bn254(d_cols, M, W, d_tree)
    root = prover.download(d_tree, (prover.merkle16_nodes(M), 4))[-1].copy()
    levels, n = 0, M
    while n > 1:
        n, levels = (n + 15) // 16, levels + 1
    top = M
    for _ in range(levels - 1):
        top = (top + 15) // 16
    out = []
    for count in COUNTS:
        idx = rng.integers(0, M, size=count, dtype=np.uint64)
        values = np.ascontiguousarray(cols[:, idx.astype(np.int64)].T)
        paths = np.zeros((count, levels, 16, 4), dtype=np.uint64)
        if levels:
            ii = np.ascontiguousarray(idx)
            prover._chk(prover.lib.zp_merkle16_open_batch_bn254(prover.ctx, d_tree.ptr, M, ii.ctypes.data, count, paths.ctypes.data))
        for o in range(3, count, 7):          # every 7th opening is corrupted, the kinds in turn
            kind, own = (o // 7) % 6, int(idx[o]) % 16
            if kind == 0 or levels == 0:
                values[o, W - 1] = (int(values[o, W - 1]) + 1) % SV.P                      # a value
            elif kind == 1:
                paths[o, 0, own, 0] ^= np.uint64(1)                                        # the own slot
            elif kind == 2:
                paths[o, levels - 1, (int(idx[o]) // 16 ** (levels - 1)) % 16 ^ 1, 1] ^= np.uint64(4)      # a sibling of the top level
            elif kind == 3 and top < 16:
                paths[o, levels - 1, 15, 0] = 1                                            # a zero slot of the short top group
            elif kind == 4 or kind == 3:
                paths[o, 0, own ^ 1] = R4                                                  # a word := r
            else:
                idx[o] = (int(idx[o]) + 1) % M                                             # the index moved
        want = np.array([SV.merkle16_verify(O.merkle16_leaf(values[o]), M, int(idx[o]), [[fr_int(w) for w in lvl] for lvl in paths[o]], fr_int(root))
                         if int(idx[o]) < M else False for o in range(count)], dtype=np.uint8)
        out.append((values, idx, paths, want))
    d_cols.free(); d_tree.free()
    _cache[(M, W)] = (root, out)
    return _cache[(M, W)]


@pytest.mark.parametrize("M,W", TREES)
def test_primitive_gives_the_checkers_flags(prover, bn_tables, form, M, W):
    root, sets = openings_of(prover, bn_tables, M, W)
    for values, idx, paths, want in sets:
        got = prover.merkle16_verify_batch_bn254(values, idx, paths, M, root)
        assert got.tolist() == want.tolist(), (M, W, len(idx))
        corrupted = list(range(3, len(idx), 7))
        assert not want[corrupted].any() and want.sum() == len(idx) - len(corrupted)
        if len(idx) >= 8:
            assert want.any() and not want.all()
    values, idx, paths, want = sets[0]
    assert prover.merkle16_verify_batch_bn254(values, [M], paths, M, root).tolist() == [0]      # an index beyond the tree is no opening of it


def gpu_case(prover, name):
    """the proof zp_stark_prove_bn128 writes for a shape of the host test"""
    from stark_verify_cases import witness
    a = BC.SHAPES[name]
    air, tr, pub = witness(name, a[0], 11)
    d_tr = prover.upload(tr)
    text = prover.stark_prove_bn128(air.name, air.program(), d_tr, [int(v) for v in pub], *a)
    d_tr.free()
    return BC.Case(name, air.program(), PR.StarkParams(*a, hash="bn128"), text)


def reference_of(prover, tables, bn_tables, name):
    """the case, its single-field mutations as texts, and per mutation the checker's class and the ctx = NULL call's answer: made once per shape"""
    key = ("case", name)
    if key not in _cache:
        case = BC.make_vair_case(BC.cpu_backend(tables, bn_tables), tables) if name == "vair" else gpu_case(prover, name)
        muts = [("honest", 0, case.proof)] + BC.single_field_mutations(case)
        rows = []
        for label, flags, m in muts:
            text = PR.proof_to_json(m)
            rows.append((label, flags, text, BC.oracle_class(case, m, tables, bn_tables, flags),
                         native.stark_verify_bn128(case.program, text, case.params, flags, bn_tables=bn_tables)))
        _cache[key] = (case, rows)
    return _cache[key]


@pytest.mark.parametrize("name", BC.NAMES)
def test_whole_proofs_get_the_checkers_class_and_the_host_calls_answer(prover, tables, bn_tables, form, name):
    case, rows = reference_of(prover, tables, bn_tables, name)
    classes = set()
    for label, flags, text, want, host in rows:
        got = native.stark_verify_bn128(case.program, text, case.params, flags, prover=prover)
        assert got[0] == want, (name, label, got, want)
        assert got == host, (name, label, got, host)
        classes.add(got[0])
    assert rows[0][3] == native.VERDICT_ACCEPT
    assert {native.VERDICT_OPENING, native.VERDICT_FRI, native.VERDICT_IDENTITY, native.VERDICT_INDICES, native.VERDICT_MALFORMED, native.VERDICT_PARAMS} <= classes


def test_batch_verdicts_through_the_ctx_and_on_the_host(prover, tables, bn_tables, form):
    if "batch" not in _cache:
        cpu = BC.cpu_backend(tables, bn_tables)
        cs = [BC.make_case("chunk16", cpu, seed) for seed in (21, 22, 23, 24, 25)]
        texts = [c.text for c in cs]
        texts[1] = PR.proof_to_json(BC.mutated(cs[1].proof, ("queries", 3, "fri", 1, "values", 5), BC.bump))
        texts[3] = PR.proof_to_json(BC.mutated(cs[3].proof, ("evals", "zw", 2, 0), BC.bump))
        _cache["batch"] = (cs[0], texts, native.stark_verify_batch_bn128(cs[0].program, texts, cs[0].params, bn_tables=bn_tables))
    case, texts, host = _cache["batch"]
    a, b = native.VERDICT_OPENING, native.VERDICT_IDENTITY
    assert host == [0, a, 0, b, 0]
    assert native.stark_verify_batch_bn128(case.program, texts, case.params, prover=prover) == [0, a, 0, b, 0]
    assert native.stark_verify_batch_bn128(case.program, texts, case.params, prover=prover, threads=3) == [0, a, 0, b, 0]


NO_TABLES = """
import sys
sys.path.insert(0, %r)
import numpy as np
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR, prover as PR
p = native.Prover(0)
air = AIR.get_air("fib")
params = PR.StarkParams(6, 1, 2, 3, 5, hash="bn128")
for call in (lambda: native.stark_verify_bn128(air.program(), "{}", params, prover=p),
             lambda: p.merkle16_verify_batch_bn254(np.zeros((1, 3), dtype=np.uint64), [0], np.zeros(0, dtype=np.uint64), 1, np.zeros(4, dtype=np.uint64))):
    try:
        call()
        print("a verdict")
    except native.ZpError as e:
        print(e.code, "not installed" in str(e))
p.close()
"""


def test_a_ctx_without_the_tables_gives_the_documented_error():
    """the tables are per device and per process: a fresh process that installs none"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", NO_TABLES % root], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:2] == ["-1 True", "-1 True"], out.stdout + out.stderr
