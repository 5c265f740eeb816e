"""Shared by tests/test_stark_verify_host.py and tests/test_gpu_stark_verify.py: the toy proofs, the mutations and the mapping from the CPU
checker's rejection messages to the verdict classes of zp_stark_verify (include/zeth_prover.h)."""
import copy
import json
import random

import numpy as np

from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR, prover as PR, verifier_air as VA
from oracle import stark_verify as SV

P = SV.P
# name -> (logn, logb, fri_logf, fri_final_log, n_queries, pow_bits)
SHAPES = {
    "fib": (6, 1, 3, 3, 5, 0),
    "perm": (8, 1, 2, 3, 6, 4),          # width 3: identity-padded leaves, stage 2
    "chunk16": (9, 1, 3, 3, 17, 8),      # stage 2 with lookup, leaf width not a multiple of 8
    "cubic": (8, 2, 3, 3, 6, 0),         # blow-up 4
    "wide32": (11, 1, 4, 2, 8, 0),       # fold by 16
}
CLASS_OF = [
    (("proof claims", "hash mode", "evaluation domain", "no soundness", "different AIR", "blow-up too small", "number of public inputs"), native.VERDICT_PARAMS),
    (("constraint identity",), native.VERDICT_IDENTITY),
    (("proof-of-work",), native.VERDICT_POW),
    (("do not follow the transcript",), native.VERDICT_INDICES),
    (("not low degree",), native.VERDICT_FINAL_DEGREE),
    (("opening does not verify",), native.VERDICT_OPENING),
    (("inconsistent",), native.VERDICT_FRI),
]


class Case:
    """one statement with an honest proof: program blob, the verifier's parameters, the proof object and its text"""

    def __init__(self, name, program, params, proof):
        self.name, self.program, self.params = name, np.ascontiguousarray(program, dtype=np.uint64), params
        self.proof = proof if isinstance(proof, dict) else json.loads(proof)
        self.text = PR.proof_to_json(self.proof)
        self.expect = SV.expectation(params.to_dict())


def witness(name, logn, seed):
    air = AIR.get_air(name)
    tr, pub = AIR.cubic_witness(logn, seed) if name == "cubic" else native.synth_trace(air.trace_kind, logn, air.width, seed)
    return air, tr, pub


def make_case(name, backend, seed=11):
    a = SHAPES[name]
    air, tr, pub = witness(name, a[0], seed)
    params = PR.StarkParams(*a[:5], pow_bits=a[5])
    return Case(name, air.program(), params, PR.prove(air, tr, pub, params, backend))


def make_vair_case(backend, rc, mds):
    """a verifier-AIR proof over one fib 2^5 proof: sparse periodic fixed columns, more than 64 public inputs (the digest path)"""
    air = AIR.get_air("fib")
    params = PR.StarkParams(5, 1, 2, 3, 3, pow_bits=0)
    tr, pub = native.synth_trace(air.trace_kind, 5, air.width, 9)
    inner = json.loads(PR.proof_to_json(PR.prove(air, tr, pub, params, backend)))
    shape = VA.Shape.of_proof(inner, 1)
    vair = VA.verifier_air(shape, rc, mds)
    wtrace, wpubs = VA.build_witness(shape, [inner], backend, air.digest_words())
    ap = VA.aggregation_params(shape, n_queries=4, fri_final_log=3)
    return Case("vair", vair.program(), ap, PR.prove(vair, wtrace, [int(v) for v in wpubs], ap, backend))


def oracle_class(case, proof, rc, mds, flags=0):
    """the verdict class of the CPU checker's answer"""
    try:
        SV.verify(proof, case.program, rc, mds, case.expect, header_only=bool(flags & native.VERIFY_HEADER_ONLY),
                  trust_openings=bool(flags & native.VERIFY_TRUST_OPENINGS))
        return native.VERDICT_ACCEPT
    except SV.Reject as e:
        for words, cls in CLASS_OF:
            if any(w in str(e) for w in words):
                return cls
        return native.VERDICT_MALFORMED
    except Exception:
        return native.VERDICT_MALFORMED


def oracle_indices(case, rc, mds):
    return SV.verify(case.proof, case.program, rc, mds, case.expect, header_only=True)["indices"]


def leaves(o, path=()):
    """(path, value) of every numeric leaf of a proof object"""
    if isinstance(o, dict):
        for k, v in o.items():
            yield from leaves(v, path + (k,))
    elif isinstance(o, list):
        for i, v in enumerate(o):
            yield from leaves(v, path + (i,))
    elif isinstance(o, int) and not isinstance(o, bool):
        yield path, o


def get(o, path):
    for k in path:
        o = o[k]
    return o


def mutated(proof, path, fn):
    """a copy of the proof with fn applied to the member at `path`; fn = None drops the member"""
    m = copy.deepcopy(proof)
    parent = get(m, path[:-1])
    if fn is None:
        del parent[path[-1]]
    else:
        parent[path[-1]] = fn(parent[path[-1]])
    return m


def bump(v):
    return (v + 1) % P


def single_field_mutations(case):
    """(label, flags, mutated proof): one field changed each"""
    pr, out = case.proof, []
    nq, n_fri = len(pr["queries"]), len(pr["fri"]["roots"])
    q = nq // 2
    add = lambda label, path, fn=bump, flags=0: out.append((label, flags, mutated(pr, path, fn)))
    trees = [("trace", ("queries", q, "trace")), ("quotient", ("queries", q, "quotient"))]
    if "stage2" in pr["roots"]:
        trees.append(("stage2", ("queries", q, "stage2")))
    trees += [("fri%d" % l, ("queries", q, "fri", l)) for l in range(n_fri)]
    for label, base in trees:
        add(label + " value", base + ("values", 0))
        add(label + " last value", base + ("values", len(get(pr, base)["values"]) - 1))
        add(label + " path word", base + ("path", 0, 1))
        add(label + " top path word", base + ("path", len(get(pr, base)["path"]) - 1, 3))
    add("index ^ 1", ("queries", q, "index"), lambda v: v ^ 1)
    if case.params.pow_bits:
        add("pow_nonce + 1", ("pow_nonce",))
        out.append(("pow_nonce dropped", 0, mutated(pr, ("pow_nonce",), None)))
    add("final-layer word", ("fri", "final", 1, 2))
    add("final-layer word, header only", ("fri", "final", 1, 2), flags=native.VERIFY_HEADER_ONLY)
    add("evaluation at zeta", ("evals", "z", 0, 1))
    add("evaluation at zeta w", ("evals", "zw", 0, 0))
    add("quotient evaluation", ("evals", "z", len(pr["evals"]["z"]) - 1, 2))
    add("trace-root word", ("roots", "trace", 2))
    add("quotient-root word", ("roots", "quotient", 0))
    add("fri-root word", ("fri", "roots", n_fri - 1, 3))
    add("public input", ("publics", 0))
    add("params.logb", ("params", "logb"))
    add("params.n_queries", ("params", "n_queries"), lambda v: v - 1)
    add("root32", ("root32",))
    add("shift", ("shift",))
    out.append(("air_digest", 0, mutated(pr, ("air_digest",), lambda d: ("0" if d[0] != "0" else "1") + d[1:])))
    out.append(("publics shortened", 0, mutated(pr, ("publics",), lambda v: v[:-1])))
    out.append(("evaluations shortened", 0, mutated(pr, ("evals", "zw"), lambda v: v[:-1])))
    out.append(("fri roots shortened", 0, mutated(pr, ("fri", "roots"), lambda v: v[:-1])))
    out.append(("final layer shortened", 0, mutated(pr, ("fri", "final", 0), lambda v: v[:-1])))
    out.append(("queries shortened", 0, mutated(pr, ("queries",), lambda v: v[:-1])))
    out.append(("queries dropped", 0, mutated(pr, ("queries",), None)))
    out.append(("queries dropped, header only", native.VERIFY_HEADER_ONLY, mutated(pr, ("queries",), None)))
    if "stage2" in pr["roots"]:
        out.append(("stage2 opening dropped", 0, mutated(pr, ("queries", q, "stage2"), None)))
        out.append(("stage2 root dropped", 0, mutated(pr, ("roots", "stage2"), None)))
    # the openings as given: what is left of the query phase is the arithmetic
    add("trace value, trusted openings", ("queries", q, "trace", "values", 0), flags=native.VERIFY_TRUST_OPENINGS)
    add("last-layer FRI value, trusted openings", ("queries", q, "fri", n_fri - 1, "values", 1), flags=native.VERIFY_TRUST_OPENINGS)
    if n_fri > 1:
        add("layer-1 FRI value, trusted openings", ("queries", q, "fri", 1, "values", 0), flags=native.VERIFY_TRUST_OPENINGS)
    add("trace path word, trusted openings", ("queries", q, "trace", "path", 0, 0), flags=native.VERIFY_TRUST_OPENINGS)
    add("trace value = p, trusted openings", ("queries", q, "trace", "values", 0), lambda v: P, flags=native.VERIFY_TRUST_OPENINGS)
    return out


def random_mutations(case, count, seed):
    """`count` proofs with one numeric leaf replaced by a uniform value below p, by p, or by 2^64 - 1"""
    rng = random.Random(seed)
    lv = list(leaves(case.proof))
    for _ in range(count):
        path, _old = lv[rng.randrange(len(lv))]
        kind = rng.randrange(3)
        new = rng.randrange(P) if kind == 0 else P if kind == 1 else (1 << 64) - 1
        yield path, new, mutated(case.proof, path, lambda v: new)
