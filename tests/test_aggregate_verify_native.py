"""zp_aggregate_verify / zp_aggregate_verify_batch with ctx = NULL: the native verifier of aggregated proofs against the checker's
(oracle/aggregate_verify.py: verify, verify_tree).  Proofs are made with the checker's backend exactly as tests/test_verifier_air.py makes them: two
chunk16 proofs at StarkParams(6, 1, 2, 3, 4, pow_bits=4), their aggregation at aggregation_params(shape, n_queries=5, fri_final_log=3), the level-2 tree
of test_aggregated_proofs_fold_again and the single-proof `fib` shape.  Per case: the return code is ZP_OK, the native verdict is ACCEPT exactly when
the checker accepts, and a rejection falls in the class the case states.  The classes follow from the documented order of the checks
(include/zeth_prover.h): a header's data that the public transcript absorbs (evaluations, final layer, nonce, long public inputs) is TRANSCRIPT --
the comparison comes before the identity at zeta, which is evaluated for all headers at the end -- and parameters are PARAMS."""
import copy
import json

import numpy as np
import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.stark import agg_statements as AS
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR
from eigen_zeth_amd.stark import verifier_air as VA
from oracle import aggregate_verify as AV
from oracle import oracle as O
from oracle import stark_verify as V
from oracle.stark_cpu import CpuBackend
from test_verifier_air import strip_paths

P = O.P
ACCEPT, MALFORMED, PARAMS, IDENTITY = native.VERDICT_ACCEPT, native.VERDICT_MALFORMED, native.VERDICT_PARAMS, native.VERDICT_IDENTITY
OPENING, TRANSCRIPT, PUBLICS, TREE = native.VERDICT_OPENING, native.VERDICT_TRANSCRIPT, native.VERDICT_PUBLICS, native.VERDICT_TREE


class World:
    """the proofs of this file, made once and never changed (every case works on a deep copy)"""

    def __init__(self, rc, mds):
        self.rc, self.mds = rc, mds
        cpu = CpuBackend(rc, mds)
        self.air = AIR.get_air("chunk16")
        self.params = PR.StarkParams(6, 1, 2, 3, 4, pow_bits=4)
        chunk = []
        for seed in (3, 4, 5, 6):
            tr, pub = native.synth_trace(self.air.trace_kind, 6, self.air.width, seed)
            chunk.append(json.loads(PR.proof_to_json(PR.prove(self.air, tr, pub, self.params, cpu))))
        self.shape1 = VA.Shape.of_proof(chunk[0], 2)
        self.vair1 = VA.verifier_air(self.shape1, rc, mds)
        self.ap1 = VA.aggregation_params(self.shape1, n_queries=5, fri_final_log=3)
        level1 = []
        for pair in (chunk[:2], chunk[2:]):
            trace, pubs = VA.build_witness(self.shape1, pair, cpu, self.air.digest_words())
            stark = json.loads(PR.proof_to_json(PR.prove(self.vair1, trace, pubs, self.ap1, cpu)))
            level1.append({"shape": self.shape1.to_dict(), "inner": [strip_paths(p) for p in pair], "stark": stark})
        self.A, self.B = level1
        self.plain = {"kind": "aggregated", "inner": self.A["inner"], "stark": self.A["stark"]}      # a level-1 text without "shape"
        self.shape2 = VA.Shape.of_proof(self.A["stark"], 2)
        self.vair2 = VA.verifier_air(self.shape2, rc, mds)
        self.ap2 = VA.aggregation_params(self.shape2, n_queries=4, fri_final_log=3)
        tr2, pubs2 = VA.build_witness(self.shape2, [self.A["stark"], self.B["stark"]], cpu, self.vair1.digest_words())
        self.top = {"shape": self.shape2.to_dict(), "level": 2, "inner": [strip_paths(self.A["stark"]), strip_paths(self.B["stark"])],
                    "children": [{"shape": self.A["shape"], "inner": self.A["inner"]}, {"shape": self.B["shape"], "inner": self.B["inner"]}],
                    "stark": json.loads(PR.proof_to_json(PR.prove(self.vair2, tr2, pubs2, self.ap2, cpu)))}
        self.programs = {self.shape1.key(): self.vair1.program(), self.shape2.key(): self.vair2.program()}
        self.statements = [(None, self.air.program(), self.params, 0), (self.shape1.to_dict(), self.vair1.program(), self.ap1, self.shape1.n_slots()),
                           (self.shape2.to_dict(), self.vair2.program(), self.ap2, self.shape2.n_slots())]
        # the single-proof shape: one `fib` proof, no grinding, identity leaves
        self.fib = AIR.get_air("fib")
        self.fib_params = PR.StarkParams(5, 1, 2, 3, 3, pow_bits=0)
        tr, pub = native.synth_trace(self.fib.trace_kind, 5, self.fib.width, 9)
        proof = json.loads(PR.proof_to_json(PR.prove(self.fib, tr, pub, self.fib_params, cpu)))
        self.fib_shape = VA.Shape.of_proof(proof, 1)
        self.fib_vair = VA.verifier_air(self.fib_shape, rc, mds)
        trace, pubs = VA.build_witness(self.fib_shape, [proof], cpu, self.fib.digest_words())
        self.fib_ap = VA.aggregation_params(self.fib_shape, n_queries=4, fri_final_log=3)
        self.fib_agg = {"shape": self.fib_shape.to_dict(), "inner": [strip_paths(proof)],
                        "stark": json.loads(PR.proof_to_json(PR.prove(self.fib_vair, trace, pubs, self.fib_ap, cpu)))}
        self.fib_statements = [(None, self.fib.program(), self.fib_params, 0), (self.fib_shape.to_dict(), self.fib_vair.program(), self.fib_ap, self.fib_shape.n_slots())]

    def checker_accepts(self, agg, leaf_params=None):
        """oracle/aggregate_verify.py on the same object: verify_tree for a text with a shape, verify for the plain level-1 form"""
        leaf_expect = V.expectation((leaf_params or self.params).to_dict())
        try:
            if "shape" not in agg:
                return bool(AV.verify(agg, self.air.program(), self.vair1.program(), self.rc, self.mds, leaf_expect, V.expectation(self.ap1.to_dict()), self.shape1.n_slots()))

            def program_of_shape(d):
                sh = VA.Shape.from_dict(d)
                return self.programs[sh.key()], sh.n_slots()

            def expect_of_shape(d):
                return V.expectation((self.ap1 if VA.Shape.from_dict(d).key() == self.shape1.key() else self.ap2).to_dict())
            return bool(AV.verify_tree(agg, self.air.program(), leaf_expect, self.rc, self.mds, program_of_shape, expect_of_shape))
        except (V.Reject, KeyError, ValueError, IndexError, TypeError):
            return False


_world = []


def get_world(tables):
    """one World per session: tests/test_agg_verify_fuzz.py takes its text from the same one"""
    if not _world:
        _world.append(World(*tables))
    return _world[0]


@pytest.fixture(scope="module")
def world(tables):
    return get_world(tables)


def test_accepts_level_one_level_two_and_the_single_proof_shape(world):
    for agg in (world.plain, world.A, world.B, world.top):
        assert native.aggregate_verify(world.statements, json.dumps(agg)) == (ACCEPT, -1)
        assert world.checker_accepts(agg)
    assert native.aggregate_verify(world.statements, json.dumps(world.top), threads=3) == (ACCEPT, -1)
    assert native.aggregate_verify(world.fib_statements, json.dumps(world.fib_agg)) == (ACCEPT, -1)
    assert AV.verify(world.fib_agg, world.fib.program(), world.fib_vair.program(), world.rc, world.mds, V.expectation(world.fib_params.to_dict()),
                     V.expectation(world.fib_ap.to_dict()), world.fib_shape.n_slots())
    # member order and whitespace of a shape dictionary do not matter
    shuffled = dict(world.A, shape=dict(reversed(list(world.A["shape"].items()))))
    assert native.aggregate_verify(world.statements, json.dumps(shuffled, indent=2)) == (ACCEPT, -1)


def _set(path, fn):
    """a mutation: walks `path` into the object and replaces the last member by fn(old)"""
    def mutate(o):
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = fn(o[path[-1]])
    return mutate


# (name, which text, mutation, expected class, expected node)
LEVEL1 = [
    ("a header that does not verify on its own", "plain", _set(("inner", 0, "evals", "z", 0, 0), lambda v: v ^ 1), TRANSCRIPT, 0),
    ("another final layer: other indices", "plain", _set(("inner", 1, "fri", "final", 0, 0), lambda v: v ^ 1), TRANSCRIPT, 0),
    ("the outer proof names proof 0's roots first", "plain", _set(("inner",), lambda v: v[::-1]), TRANSCRIPT, 0),
    ("a header with openings", "plain", lambda o: o["inner"][0].__setitem__("queries", []), TREE, 0),
    ("another E_zw", "plain", _set(("inner", 1, "evals", "zw", 3, 2), lambda v: v ^ 1), TRANSCRIPT, 0),
    ("another nonce than the circuit hashed", "plain", _set(("inner", 0, "pow_nonce"), lambda v: v ^ 1), TRANSCRIPT, 0),
    ("one public input too many", "plain", _set(("stark", "publics"), lambda v: list(v) + [0]), PARAMS, -1),
    ("one query opening of the outer STARK flipped", "A", _set(("stark", "queries", 1, "trace", "values", 0), lambda v: v ^ 1), OPENING, -1),
    ("one path word flipped", "A", _set(("stark", "queries", 2, "quotient", "path", 1, 2), lambda v: v ^ 1), OPENING, -1),
    ("an outer evaluation flipped", "A", _set(("stark", "evals", "z", 1, 0), lambda v: v ^ 1), IDENTITY, -1),
    ("a root of an inner proof", "A", _set(("inner", 1, "roots", "quotient", 2), lambda v: v ^ 1), TRANSCRIPT, 0),
]
LEVEL2 = [
    ("a chunk proof at a leaf", _set(("children", 1, "inner", 0, "evals", "z", 2, 1), lambda v: v ^ 1), TRANSCRIPT, 2),
    ("children under the wrong parents", _set(("children",), lambda v: v[::-1]), TRANSCRIPT, 1),
    ("an aggregation STARK claiming other public inputs", _set(("inner", 0, "publics", 3), lambda v: (v + 1) % P), TRANSCRIPT, 0),
    ("the chunk proofs withheld", lambda o: o.__delitem__("children"), PARAMS, 0),
    ("one child too few", _set(("children",), lambda v: v[:1]), TREE, 0),
    ("children of mixed shapes", lambda o: o["children"][1]["shape"].__setitem__("n_queries", 5), TREE, 0),
]


@pytest.mark.parametrize("name,which,mutate,cls,node", LEVEL1, ids=[c[0] for c in LEVEL1])
def test_level_one_mutations_are_rejected_in_their_class(world, name, which, mutate, cls, node):
    bad = copy.deepcopy(getattr(world, which))
    mutate(bad)
    assert native.aggregate_verify(world.statements, json.dumps(bad)) == (cls, node)
    assert not world.checker_accepts(bad)


def test_fewer_inner_queries_than_the_verifier_requires(world):
    want5 = PR.StarkParams(6, 1, 2, 3, 5, pow_bits=4)
    st = [(None, world.air.program(), want5, 0)] + world.statements[1:]
    assert native.aggregate_verify(st, json.dumps(world.plain)) == (PARAMS, 0)
    assert not world.checker_accepts(world.plain, leaf_params=want5)


@pytest.mark.parametrize("name,mutate,cls,node", LEVEL2, ids=[c[0] for c in LEVEL2])
def test_level_two_mutations_are_rejected_in_their_class(world, name, mutate, cls, node):
    bad = copy.deepcopy(world.top)
    mutate(bad)
    assert native.aggregate_verify(world.statements, json.dumps(bad)) == (cls, node)
    assert not world.checker_accepts(bad)


def test_a_shape_absent_from_the_table_is_a_verdict(world):
    assert native.aggregate_verify(world.statements[:2], json.dumps(world.top)) == (PARAMS, -1)      # the top shape
    st = [world.statements[0], world.statements[2]]
    assert native.aggregate_verify(st, json.dumps(world.top)) == (PARAMS, 0)                          # the children's shape
    assert native.aggregate_verify(world.statements[1:], json.dumps(world.A)) == (PARAMS, 0)          # no leaf statement


def test_children_nested_nine_deep_are_refused(world):
    def nest(levels):
        """a chain of nodes with one header and one child each, `levels` "children" lists below the top node"""
        node = {"shape": world.top["shape"], "inner": world.top["inner"][:1]}
        for _ in range(levels):
            node = {"shape": world.top["shape"], "inner": world.top["inner"][:1], "children": [node]}
        return dict(node, stark=world.top["stark"])
    for levels in (8, 9):                                  # nine and ten levels of nodes
        deep = nest(levels)
        assert native.aggregate_verify(world.statements, json.dumps(deep)) == (TREE, -1)
        assert not world.checker_accepts(deep)
    # eight levels of nodes are walked: the verdict comes from the first node that fails -- the top node's header is an aggregation STARK over the
    # chunk verifier AIR, not a proof of its child's shape
    assert native.aggregate_verify(world.statements, json.dumps(nest(7))) == (PARAMS, 0)


def test_header_only_skips_the_outer_openings_alone(world):
    flipped = copy.deepcopy(world.top)
    flipped["stark"]["queries"][0]["trace"]["path"][0][0] ^= 1
    assert native.aggregate_verify(world.statements, json.dumps(flipped)) == (OPENING, -1)
    assert native.aggregate_verify(world.statements, json.dumps(flipped), native.VERIFY_HEADER_ONLY) == (ACCEPT, -1)
    assert native.aggregate_verify(world.statements, json.dumps(world.top), native.VERIFY_HEADER_ONLY) == (ACCEPT, -1)
    for name, mutate, cls, node in LEVEL2:
        bad = copy.deepcopy(world.top)
        mutate(bad)
        assert native.aggregate_verify(world.statements, json.dumps(bad), native.VERIFY_HEADER_ONLY) == (cls, node), name
    bad = copy.deepcopy(world.top)
    bad["stark"]["evals"]["z"][1][0] ^= 1
    assert native.aggregate_verify(world.statements, json.dumps(bad), native.VERIFY_HEADER_ONLY) == (IDENTITY, -1)


def test_batch_gives_mixed_verdicts(world):
    bad = copy.deepcopy(world.top)
    bad["children"][0]["inner"][1]["fri"]["roots"][0][1] ^= 1
    texts = [json.dumps(world.top), json.dumps(bad), json.dumps(world.A)]
    got = native.aggregate_verify_batch(world.statements, texts, threads=2)
    assert got[0] == ACCEPT and got[1] == TRANSCRIPT and got[2] == ACCEPT
    assert native.aggregate_verify(world.statements, texts[1]) == (TRANSCRIPT, 1)


def test_text_outside_the_grammar_is_malformed_not_an_error(world):
    good = json.dumps(world.top)
    for text in (good[:len(good) // 2], good[:-1], "", "[]", good + "x"):
        assert native.aggregate_verify(world.statements, text) == (MALFORMED, -1)
    for mutate in (_set(("inner",), lambda v: 5), _set(("inner", 0, "roots", "trace"), lambda v: 7), _set(("children",), lambda v: {"a": 1}),
                   _set(("shape", "n_queries"), lambda v: 10 ** 9), _set(("shape", "n_pub_inner"), lambda v: 10 ** 30), _set(("shape", "logn"), lambda v: -1),
                   _set(("children", 0, "shape", "W"), lambda v: 1 << 40), lambda o: o["shape"].__delitem__("pow_bits"), _set(("stark",), lambda v: [1, 2])):
        bad = copy.deepcopy(world.top)
        mutate(bad)
        assert native.aggregate_verify(world.statements, json.dumps(bad))[0] == MALFORMED
    no_stark = {k: v for k, v in world.top.items() if k != "stark"}
    assert native.aggregate_verify(world.statements, json.dumps(no_stark)) == (MALFORMED, -1)


def test_the_callers_mistakes_are_negative_codes(world):
    import ctypes as C
    lib = native.load_library()
    text = json.dumps(world.A).encode()
    table, keep = native.agg_statements(world.statements)
    verdict, where = C.c_int32(-5), C.c_int32(-5)
    assert lib.zp_aggregate_verify(None, table, len(table), text, len(text), 0, 0, C.byref(verdict), C.byref(where)) == 0 and verdict.value == ACCEPT
    assert lib.zp_aggregate_verify(None, None, len(table), text, len(text), 0, 0, C.byref(verdict), C.byref(where)) == -1
    assert lib.zp_aggregate_verify(None, table, len(table), None, 0, 0, 0, C.byref(verdict), C.byref(where)) == -1
    assert lib.zp_aggregate_verify(None, table, len(table), text, len(text), 0, 0, None, C.byref(where)) == -1
    assert lib.zp_aggregate_verify(None, table, len(table), text, len(text), native.VERIFY_TRUST_OPENINGS, 0, C.byref(verdict), C.byref(where)) == -1
    assert lib.zp_aggregate_verify(None, table, 0, text, len(text), 0, 0, C.byref(verdict), C.byref(where)) == -1
    assert lib.zp_aggregate_verify_batch(None, table, len(table), None, None, 1, 0, 0, None) == -1
    for bad_statements in ([(None, np.zeros(40, dtype=np.uint64), world.params, 0)] + world.statements[1:],                     # no program blob
                           [world.statements[0], (world.shape1.to_dict(), world.vair1.program()[:-3], world.ap1, world.shape1.n_slots())],      # truncated
                           world.statements + [world.statements[0]],                                                            # two leaf statements
                           [world.statements[0], ({"logn": 3}, world.vair1.program(), world.ap1, 4)],                           # no shape dictionary
                           [world.statements[0], (world.shape1.to_dict(), world.vair1.program(), world.ap1, 0)]):               # no query slots
        with pytest.raises(native.ZpError):
            native.aggregate_verify(bad_statements, text)


def test_statement_table_file_round_trips_through_the_compiled_host(world, tmp_path):
    """eigen_zeth_amd/stark/agg_statements.py writes what host/verify_chunk reads in its `aggregated` mode: the verdict of a compiled host, no GPU"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "verify_chunk")
    assert os.path.exists(exe), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    st = AS.statements_for(world.top, world.air.program(), world.params, lambda sh: world.ap1 if sh.key() == world.shape1.key() else world.ap2, world.rc, world.mds)
    assert [s[0] for s in st] == [None, world.shape2.to_dict(), world.shape1.to_dict()]
    table, good, bad = str(tmp_path / "statements.bin"), str(tmp_path / "good.json"), str(tmp_path / "bad.json")
    AS.write_table(table, st)
    tampered = copy.deepcopy(world.top)
    tampered["children"][1]["inner"][0]["evals"]["z"][2][1] ^= 1
    open(good, "w").write(json.dumps(world.top))
    open(bad, "w").write(json.dumps(tampered))
    out = subprocess.run([exe, "aggregated", table, good, "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "verdict 0 accept where -1", out.stdout + out.stderr
    out = subprocess.run([exe, "aggregated", table, bad, "host", "header-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and out.stdout.strip() == "verdict 9 transcript where 2", out.stdout + out.stderr
