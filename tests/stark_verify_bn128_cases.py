"""Shared by tests/test_stark_verify_bn128_host.py and tests/test_gpu_stark_verify_bn128.py: BN128-hash-mode proofs (16-ary Poseidon-BN254 trees,
transcript over F_r) of the toy statements, their mutations and the CPU checker's class for each (oracle/stark_verify.py with
expect["hash"] == "bn128").  A field element of F_r stands in the proof as a quoted decimal; an opened value or an evaluation as a number."""
import json
import random

import numpy as np

from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR, prover as PR, verifier_air as VA
from oracle import stark_verify as SV
from stark_verify_cases import CLASS_OF, get, mutated, witness

P, R = SV.P, SV.R_BN254
# name -> (logn, logb, fri_logf, fri_final_log, n_queries)
SHAPES = {
    "fib": (6, 1, 2, 3, 5),
    "perm": (8, 1, 2, 3, 6),             # stage 2
    "chunk16": (7, 1, 3, 3, 6),          # stage 2 with lookup
    "cubic": (8, 2, 3, 3, 6),            # blow-up 4
    "wide64": (7, 1, 4, 2, 6),           # 64 columns: a two-block leaf sponge, g = 0, fold by 16, 48-value FRI leaves
}
NAMES = list(SHAPES) + ["vair"]


class Case:
    def __init__(self, name, program, params, proof):
        self.name, self.program, self.params = name, np.ascontiguousarray(program, dtype=np.uint64), params
        self.proof = proof if isinstance(proof, dict) else json.loads(proof)
        self.text = PR.proof_to_json(self.proof)
        self.expect = SV.expectation(params.to_dict())
        assert self.expect["hash"] == "bn128"


def cpu_backend(tables, bn_tables):
    from oracle.stark_cpu import CpuBackend
    return CpuBackend(*tables, hash_mode="bn128", bn_tables=bn_tables)


def make_case(name, backend, seed=11):
    a = SHAPES[name]
    air, tr, pub = witness(name, a[0], seed)
    params = PR.StarkParams(*a, hash="bn128")
    return Case(name, air.program(), params, PR.prove(air, tr, pub, params, backend))


def make_vair_case(backend, tables):
    """a verifier-AIR proof, in BN128 mode, over one Goldilocks-mode fib 2^5 proof: 47 columns, sparse periodic fixed columns, and more than 64
    public inputs -- the 16-ary commitment of the public inputs"""
    from oracle.stark_cpu import CpuBackend
    gl = CpuBackend(*tables)
    air = AIR.get_air("fib")
    params = PR.StarkParams(5, 1, 2, 3, 3, pow_bits=0)
    tr, pub = native.synth_trace(air.trace_kind, 5, air.width, 9)
    inner = json.loads(PR.proof_to_json(PR.prove(air, tr, pub, params, gl)))
    shape = VA.Shape.of_proof(inner, 1)
    vair = VA.verifier_air(shape, *tables)
    wtrace, wpubs = VA.build_witness(shape, [inner], gl, air.digest_words())
    ap = VA.aggregation_params(shape, n_queries=4, fri_final_log=3, hash="bn128")
    return Case("vair", vair.program(), ap, PR.prove(vair, wtrace, [int(v) for v in wpubs], ap, backend))


def oracle_class(case, proof, tables, bn_tables, flags=0):
    """the verdict class of the CPU checker's answer"""
    try:
        SV.verify(proof, case.program, *tables, case.expect, bn_tables, header_only=bool(flags & native.VERIFY_HEADER_ONLY),
                  trust_openings=bool(flags & native.VERIFY_TRUST_OPENINGS))
        return native.VERDICT_ACCEPT
    except SV.Reject as e:
        for words, cls in CLASS_OF:
            if any(w in str(e) for w in words):
                return cls
        return native.VERDICT_MALFORMED
    except Exception:
        return native.VERDICT_MALFORMED


def oracle_indices(case, tables, bn_tables):
    return SV.verify(case.proof, case.program, *tables, case.expect, bn_tables, header_only=True)["indices"]


def is_fr(v):
    return isinstance(v, str) and v.isdigit()


def leaves(o, path=()):
    """(path, value) of every number of a proof object: the ints and the quoted digit strings"""
    if isinstance(o, dict):
        for k, v in o.items():
            yield from leaves(v, path + (k,))
    elif isinstance(o, list):
        for i, v in enumerate(o):
            yield from leaves(v, path + (i,))
    elif (isinstance(o, int) and not isinstance(o, bool)) or (is_fr(o) and path[0] != "air_digest"):
        yield path, o


def bump(v):
    return str((int(v) + 1) % R) if isinstance(v, str) else (v + 1) % P


def tree_shapes(case):
    """per opened tree: (label, key path inside a query, leaf count, log2 of the rows per leaf, columns)"""
    pr, p = case.proof, case.params
    logm = p.logn + p.logb
    M = 1 << logm
    W, W2 = int(case.program[1]), int(case.program[2])      # the program blob's header: trace and stage-2 widths
    Wq = len(pr["evals"]["z"]) - len(pr["evals"]["zw"])
    out = []
    for label, key, width in (("trace", ("trace",), W), ("stage2", ("stage2",), W2), ("quotient", ("quotient",), Wq)):
        if not width:
            continue
        g = SV.bn128_rows_per_leaf_log(width, logm)
        out.append((label, key, M >> g, g, width))
    sched, _ = SV.fri_schedule(p.logn, p.logb, p.fri_logf, p.fri_final_log)
    for l, (lg, f) in enumerate(sched):
        out.append(("fri%d" % l, ("fri", l), 1 << (lg - f), 0, 3 << f))
    return out


def single_field_mutations(case):
    """(label, flags, mutated proof): one field changed each"""
    pr, out = case.proof, []
    p = case.params
    logm = p.logn + p.logb
    nq, n_fri = len(pr["queries"]), len(pr["fri"]["roots"])
    q = nq // 2
    j = pr["queries"][q]["index"]
    add = lambda label, path, fn=bump, flags=0: out.append((label, flags, mutated(pr, path, fn)))
    for label, key, n_leaves, g, width in tree_shapes(case):
        base = ("queries", q) + key
        op = get(pr, base)
        pos = j & (n_leaves - 1) if not label.startswith("fri") else None
        if pos is None:      # the row a FRI layer opens: the index folded down layer by layer
            pos, sched = j, SV.fri_schedule(p.logn, p.logb, p.fri_logf, p.fri_final_log)[0]
            for (lg, f) in sched[:int(label[3:]) + 1]:
                pos &= (1 << (lg - f)) - 1
        add(label + " value", base + ("values", 0))
        add(label + " last value", base + ("values", len(op["values"]) - 1))
        if op["path"]:
            own = pos % 16
            add(label + " sibling word", base + ("path", 0, own ^ 1))
            add(label + " own-slot word", base + ("path", 0, own))
            add(label + " top-level word", base + ("path", len(op["path"]) - 1, 0))
            add(label + " path word = r", base + ("path", 0, own ^ 1), lambda v: str(R))
            # a short top group: the children beyond the level's size are zero and must stay zero
            n = n_leaves
            for _ in range(len(op["path"]) - 1):
                n = (n + 15) // 16
            if n < 16:
                add(label + " zero slot := 1", base + ("path", len(op["path"]) - 1, 15), lambda v: "1")
    add("trace root", ("roots", "trace", 0))
    add("quotient root", ("roots", "quotient", 0))
    add("trace root = r", ("roots", "trace", 0), lambda v: str(R))
    add("fri root", ("fri", "roots", n_fri - 1, 0))
    add("fri root = r", ("fri", "roots", 0, 0), lambda v: str(R))
    add("evaluation at zeta", ("evals", "z", 0, 1))
    add("evaluation at zeta w", ("evals", "zw", 0, 0))
    add("final-layer word", ("fri", "final", 1, 2))
    add("final-layer word, header only", ("fri", "final", 1, 2), flags=native.VERIFY_HEADER_ONLY)
    add("public input", ("publics", 0))
    add("params.logb", ("params", "logb"))
    add("params.pow_bits", ("params", "pow_bits"))
    add("root32", ("root32",))
    add("hash relabelled gl", ("params", "hash"), lambda v: "gl")
    add("index ^ 1", ("queries", q, "index"), lambda v: v ^ 1)
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
    # the openings as given.  A grouped leaf holds 2^g rows: only the queried row's values enter the arithmetic
    label, key, n_leaves, g, width = tree_shapes(case)[0]
    mine = j >> (logm - g)
    add("trace value of the queried row, trusted openings", ("queries", q, "trace", "values", (0 << g) + mine), flags=native.VERIFY_TRUST_OPENINGS)
    if g:
        add("trace value of another row, trusted openings", ("queries", q, "trace", "values", (0 << g) + (mine ^ 1)), flags=native.VERIFY_TRUST_OPENINGS)
    add("last-layer FRI value, trusted openings", ("queries", q, "fri", n_fri - 1, "values", 1), flags=native.VERIFY_TRUST_OPENINGS)
    add("trace path word, trusted openings", ("queries", q, "trace", "path", 0, 0), flags=native.VERIFY_TRUST_OPENINGS)
    add("trace value = p, trusted openings", ("queries", q, "trace", "values", 0), lambda v: P, flags=native.VERIFY_TRUST_OPENINGS)
    return out


def random_mutations(case, outside, inside, seed):
    """`outside` proofs with one number outside "queries" replaced, then `inside` with one inside it (unstratified draws land in the openings nine
    times out of ten).  A number becomes a uniform value of its field, the field's modulus, or 2^64 - 1 (a field element of F_r: 2^256 - 1)"""
    rng = random.Random(seed)
    lv = list(leaves(case.proof))
    pools = [[x for x in lv if x[0][0] != "queries"], [x for x in lv if x[0][0] == "queries"]]
    for pool, count in zip(pools, (outside, inside)):
        for _ in range(count):
            path, old = pool[rng.randrange(len(pool))]
            kind = rng.randrange(3)
            if isinstance(old, str):
                new = str(rng.randrange(R) if kind == 0 else R if kind == 1 else (1 << 256) - 1)
            else:
                new = rng.randrange(P) if kind == 0 else P if kind == 1 else (1 << 64) - 1
            yield path, new, mutated(case.proof, path, lambda v: new)
