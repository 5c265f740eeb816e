"""What tests/test_witness_check_host.py and tests/test_gpu_witness_check.py share: the checker's own verdict on a (program, trace) pair and the case
set.  TEST INFRASTRUCTURE.

The expectation is oracle/air_program.py's row evaluator, Program.evaluate_base, with the operand rules of include/zeth_prover.h
(zp_stark_check_witness): next row = (r + 1) mod N, fixed column 0 = [r = 0], 1 = [r = N - 1], j >= 2 = fixed_period(j - 2)[r mod 2^lp], kind 6 =
w^r - w^(N-1) with w = NV.root(logn).  evaluate_base's operations are `(a + b) % P` and the like, so it takes ALL rows in one call when every
operand is a numpy array of Python ints (dtype=object) -- the same walk, row by row inside numpy (test_vector_walk_is_the_row_walk pins that to
the row-at-a-time call).  Stage-2 columns come from their header definitions with oracle.naive's F_{p^3} functions, one shared inversion."""
import functools

import numpy as np

import program_cases as PC
from oracle import naive as NV
from oracle.air_program import Program

P = NV.P
NONE = (1 << 64) - 1
SATISFIED, VIOLATED, NONCANONICAL = 0, 1, 2


def derived_challenge(prog):
    g = prog.digest_words()[:3]
    if g[1] == 0 and g[2] == 0:
        g[1] = 1
    return g


def _batch_inverse(dens):
    """1 / d for F_{p^3} values d (Montgomery's trick: one NV.e3_inv)"""
    pre, run = [], [1, 0, 0]
    for d in dens:
        pre.append(run)
        run = NV.e3_mul(run, d)
    inv = NV.e3_inv(run)
    out = [None] * len(dens)
    for i in range(len(dens) - 1, -1, -1):
        out[i] = NV.e3_mul(inv, pre[i])
        inv = NV.e3_mul(inv, dens[i])
    return out


def stage2_columns(prog, tr, g):
    """the W2 stage-2 columns (lists of N ints) of a trace: Z[0] = 1, Z[i+1] = Z[i] (a[i] + g) / (b[i] + g);  h1 = 1 / (a + g), h2 = m / (t + g),
    S[0] = 0, S[i+1] = S[i] + h1[i] - h2[i]"""
    cols = []
    sh = lambda v: [(int(v) + g[0]) % P, g[1], g[2]]
    for s in prog.stage2:
        a, b, m = tr[s["a"]], tr[s["b"]], tr[s["m"]]
        if s["kind"] == 1:
            binv = _batch_inverse([sh(v) for v in b])
            z, rows = [1, 0, 0], []
            for ai, bi in zip(a, binv):
                rows.append(z)
                z = NV.e3_mul(z, NV.e3_mul(sh(ai), bi))
            cols += [[r[c] for r in rows] for c in range(3)]
        else:
            ainv, tinv = _batch_inverse([sh(v) for v in a]), _batch_inverse([sh(v) for v in b])
            acc, rows = [0, 0, 0], []
            for h1, ti, mi in zip(ainv, tinv, m):
                h2 = [v * int(mi) % P for v in ti]
                rows.append(h1 + h2 + acc)
                acc = [(acc[c] + h1[c] - h2[c]) % P for c in range(3)]
            cols += [[r[k] for r in rows] for k in range(9)]
    return cols


def row_operands(prog, trace, pubs, logn, chal=None):
    """(columns incl. stage 2, fixed columns, publics + challenge, xml) as object arrays over all N rows"""
    N = 1 << logn
    obj = lambda v: np.array([int(x) for x in v], dtype=object)
    tr = [obj(c) for c in np.asarray(trace, dtype=np.uint64).reshape(prog.width, N)]
    pubchal = [int(v) for v in pubs]
    if prog.stage2:
        g = [int(v) for v in chal] if chal is not None else derived_challenge(prog)
        tr += [obj(c) for c in stage2_columns(prog, tr, g)]
        pubchal += g
    rows = np.arange(N)
    fixed = [obj(rows == 0), obj(rows == N - 1)]
    for k, (lp, _) in enumerate(prog.fixed_cols):
        fixed.append(obj(prog.fixed_period(k, pubs) * (N >> lp)))
    w = NV.root(logn)
    x, xs = 1, []
    for _ in range(N):
        xs.append(x)
        x = x * w % P
    xml = obj([(v - xs[N - 1]) % P for v in xs])
    return tr, fixed, pubchal, xml


def oracle_outs(blob, trace, pubs, logn, chal=None):
    """int array [K][N]: constraint k at row r"""
    prog = Program(blob)
    N = 1 << logn
    tr, fixed, pubchal, xml = row_operands(prog, trace, pubs, logn, chal)
    outs = prog.evaluate_base(tr, [np.roll(c, -1) for c in tr], fixed, pubchal, xml)
    return [np.asarray(o, dtype=object) if np.ndim(o) else np.array([int(o)] * N, dtype=object) for o in outs]


def oracle_report(blob, trace, pubs, logn, chal=None):
    """(report[8], counts[K], first_rows[K]) as lists of ints -- what zp_stark_check_witness must write, word for word"""
    prog = Program(blob)
    N, K = 1 << logn, prog.n_constraints
    flat = np.asarray(trace, dtype=np.uint64).reshape(-1)
    bad = np.nonzero(flat >= np.uint64(P))[0]
    if len(bad):
        return [NONCANONICAL, NONE, NONE, 0, 0, len(bad), int(bad[0]) // N, int(bad[0]) % N], [0] * K, [NONE] * K
    counts, first = [], []
    for o in oracle_outs(blob, trace, pubs, logn, chal):
        nz = np.nonzero(o != 0)[0]
        counts.append(len(nz))
        first.append(int(nz[0]) if len(nz) else NONE)
    total = sum(counts)
    row = min(first)
    return [VIOLATED if total else SATISFIED, row, first.index(row) if total else NONE, total, sum(c != 0 for c in counts), 0, NONE, NONE], counts, first


def violated_pairs(blob, trace, pubs, logn, chal=None):
    """the set of (constraint, row) the checker finds violated"""
    return {(k, int(r)) for k, o in enumerate(oracle_outs(blob, trace, pubs, logn, chal)) for r in np.nonzero(o != 0)[0]}


# ---- inputs
def random_inputs(shape, logn, seed):
    """a seeded canonical trace and publics for a program of tests/program_cases.py"""
    rng = np.random.default_rng(seed)
    draw = lambda n: (rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)) % np.uint64(P)
    return draw(shape["width"] << logn).reshape(shape["width"], 1 << logn), [int(v) for v in draw(shape["n_pub"])]


@functools.lru_cache(maxsize=None)
def random_case(name, logn):
    """(blob, trace, pubs, oracle's (report, counts, first rows)) of one entry of program_cases.CASES on 2^logn rows; computed once per session"""
    blob, shape = PC.case(name, logn)
    seed = [c[1] for c in PC.CASES if c[0] == name][0]
    trace, pubs = random_inputs(shape, logn, 7000 + 31 * seed + logn)
    return blob, trace, pubs, oracle_report(blob, trace, pubs, logn)


SATISFIED_AIRS = ("fib", "wide8", "perm", "chunk16", "cubic", "periodic")
EXPLICIT_CHALLENGE = [0x1234567890ABCDEF % P, 0x0FEDCBA987654321, 77]


@functools.lru_cache(maxsize=None)
def honest_case(name, logn):
    """(air, program blob, trace, publics) of a built-in AIR with its own witness"""
    from eigen_zeth_amd import native
    from eigen_zeth_amd.stark import air as AIR
    if name == "cubic":
        air = AIR.get_air("cubic")
        tr, pub = AIR.cubic_witness(logn, 5)
    elif name == "periodic":
        air = AIR.periodic_air(logn)
        tr, pub = AIR.periodic_witness(logn, 6)
    else:
        air = AIR.get_air(name)
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 11 + logn)
    tr.setflags(write=False)
    return air, np.ascontiguousarray(air.program(), dtype=np.uint64), tr, [int(v) for v in pub]


def flipped(trace, col, row, delta=1):
    t = np.array(trace, dtype=np.uint64)
    t[col, row] = (int(t[col, row]) + delta) % P
    return t


def broken_perm(logn):
    """perm with b no permutation of a (c = a^2 kept): one b cell takes a value a does not hold"""
    air, blob, tr, pub = honest_case("perm", logn)
    t = np.array(tr, dtype=np.uint64)
    have = {int(v) for v in t[0]}
    v = 12345
    while v in have:
        v += 1
    t[1, 3 % (1 << logn)] = v
    return blob, t, pub


def broken_lookup(logn, name="chunk16"):
    """chunk AIR with one range value r outside the table; q (the permutation of r), c = r^2 and d = fa r + fb follow it, so only the lookup breaks"""
    air, blob, tr, pub = honest_case(name, logn)
    t = np.array(tr, dtype=np.uint64)
    Ww = air.width - 8
    fa, fb, r, q, tt, c, d = Ww, Ww + 1, Ww + 2, Ww + 3, Ww + 4, Ww + 6, Ww + 7
    row = 5 % (1 << logn)
    old, new = int(t[r, row]), int(max(int(v) for v in t[tt])) + 9
    t[r, row] = new
    t[q, int(np.nonzero(t[q] == np.uint64(old))[0][0])] = new
    t[c, row] = new * new % P
    t[d, row] = (int(t[fa, row]) * new + int(t[fb, row])) % P
    return blob, t, pub


@functools.lru_cache(maxsize=None)
def verifier_air_case():
    """(program blob, trace, publics, logn) of a recursion STARK's statement: the verifier AIR over one tiny chunk proof made by the checker's CPU
    backend -- 47 columns, ~100 sparse periodic fixed columns with public-input entries, 120 constraints on 2^12 rows"""
    import json
    from eigen_zeth_amd import native
    from eigen_zeth_amd.poseidon_constants import default_mds, default_round_constants
    from eigen_zeth_amd.stark import air as AIR, prover as PR, verifier_air as VA
    from oracle.stark_cpu import CpuBackend
    rc, mds = np.array(default_round_constants(), dtype=np.uint64), np.array(default_mds(), dtype=np.uint64)
    cpu = CpuBackend(rc, mds)
    air = AIR.get_air("fib")
    tr, pub = native.synth_trace(air.trace_kind, 5, air.width, 9)
    proof = json.loads(PR.proof_to_json(PR.prove(air, tr, pub, PR.StarkParams(5, 1, 2, 3, 3, pow_bits=0), cpu)))
    shape = VA.Shape.of_proof(proof, 1)
    vair = VA.verifier_air(shape, rc, mds)
    wtrace, pubs = VA.build_witness(shape, [proof], cpu, air.digest_words())
    wtrace = np.ascontiguousarray(wtrace, dtype=np.uint64)
    wtrace.setflags(write=False)
    return np.ascontiguousarray(vair.program(), dtype=np.uint64), wtrace, [int(v) for v in pubs], shape.logn_trace()
