"""Seeded generator of well-formed ZPAIR1 constraint programs (the blob of include/zeth_prover.h, "N4 as data") and the fixed
case set the interpreter tests walk: tests/test_program_cases.py (no GPU) and tests/test_gpu_program_cases.py.

Plain Python + numpy.  Nothing here imports the product package or the checker: the words are written straight from the header's
layout, so a blob of this module is what a foreign host (the Rust prover service) could hand over -- not what
stark/air.py: compile_program happens to emit.  What makes a blob well-formed, and what the generator therefore keeps:
  * a slot is read only after an earlier instruction wrote it (the GPU interpreter's slot file is not zeroed);
  * every index lies inside its limit as zp_eval_quotient_rows checks it; constants and entry values are < p;
  * the OUT count is header word 8; no stage-2 table, no stage-2 columns, no challenges;
  * the destination field and the second operand of an OUT hold ARBITRARY bits: every reader must ignore them.
bounded=True tracks a degree (a, b) per slot the way stark/air.py: degree does (value of degree <= a (N - 1) + b) and never forms
a product above a = 3, b = 2: every constraint stays below 4 N, so a quotient with blow-up 4 can be interpolated."""
import numpy as np

P = 0xFFFFFFFF00000001
MAGIC = int.from_bytes(b"ZPAIR1\0\0", "little")
HEADER_WORDS = 12
OP_ADD, OP_SUB, OP_MUL, OP_OUT = 1, 2, 3, 4
K_SLOT, K_COL, K_COLN, K_FIXED, K_PUB, K_CONST, K_XML = range(7)
SPECIAL_CONSTS = [0, 1, P - 1, P - 2, 1 << 32, (1 << 32) - 1]
FILLS = ("empty", "full", "pub", "rand")
MAX_DEG = (3, 2)


def instr_word(op, dst, ka, ia, kb, ib):
    return op | (dst << 8) | (ka << 24) | (ia << 28) | (kb << 44) | (ib << 48)


def _field(rng):
    while True:
        v = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        if v < P:
            return v


def _index(rng, limit):
    """an index below limit; the two ends come up often"""
    r = int(rng.integers(0, 4))
    return limit - 1 if r == 0 else 0 if r == 1 else int(rng.integers(0, limit))


def _sparse_column(rng, lp, n_pub, fill):
    """[(pos, is_pub, value or public index)]: distinct positions in no particular order"""
    p = 1 << lp
    if fill == "empty":
        return []
    n = p if fill in ("full", "pub") else int(rng.integers(0, p + 1))
    ent = []
    for pos in rng.permutation(p)[:n].tolist():
        is_pub = n_pub > 0 and (fill == "pub" or (fill == "rand" and int(rng.integers(0, 3)) == 0))
        if is_pub:
            ent.append((pos, True, _index(rng, n_pub)))
        else:
            ent.append((pos, False, [P - 1, 1, _field(rng), _field(rng)][int(rng.integers(0, 4))]))
    if fill in ("full", "rand") and ent and all(e[1] for e in ent):
        ent[0] = (ent[0][0], False, P - 1)
    return ent


def gen(seed, logn=7, *, width=3, n_pub=4, n_const=6, n_slots=8, K=4, n_body=24, lps=(), fills=None, cover=False, bounded=False):
    """(blob uint64[], shape): one well-formed program.  lps: period logs of the sparse fixed columns, "n" = logn (an int above logn
    is clamped to it); fills: per sparse column one of FILLS (default: seeded choice).  cover=True walks every (op, kind a, kind b) of
    add / sub / mul and every operand kind under OUT before it goes on at random.  The instruction stream does not depend on logn."""
    rng = np.random.default_rng(seed)
    lp = [logn if v == "n" else min(int(v), logn) for v in lps]
    n_fixed = 2 + len(lp)
    limit = {K_COL: width, K_COLN: width, K_FIXED: n_fixed, K_PUB: n_pub, K_CONST: n_const, K_XML: 1}
    leaf_deg = {K_COL: (1, 0), K_COLN: (1, 0), K_FIXED: (1, 0), K_PUB: (0, 0), K_CONST: (0, 0), K_XML: (0, 1)}
    leaves = [k for k in sorted(limit) if limit[k] > 0]
    assert width >= 1 and n_slots >= 1 and K >= 1 and n_body >= 1
    consts = [SPECIAL_CONSTS[i] if i < len(SPECIAL_CONSTS) else (SPECIAL_CONSTS[i % 6] if i % 5 == 0 else _field(rng)) for i in range(n_const)]
    deg = {}                                     # written slot -> degree

    def operand(kind=None):
        if kind is None:
            kinds = leaves + ([K_SLOT] * 3 if deg else [])
            kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == K_SLOT:
            s = sorted(deg)[int(rng.integers(0, len(deg)))]
            return kind, s, deg[s]
        return kind, _index(rng, limit[kind]), leaf_deg[kind]

    todo = []
    if cover:
        assert n_pub > 0 and n_const > 0
        todo = [(op, ka, kb) for op in (OP_ADD, OP_SUB, OP_MUL) for ka in range(7) for kb in range(7)]
        todo = [todo[i] for i in rng.permutation(len(todo)).tolist()]
        n_body = max(n_body, len(todo) + 1)
    out_kinds = list(rng.permutation(7).tolist()) if cover else []
    assert not out_kinds or K >= 7
    words, body_left, out_left = [], n_body, K
    while body_left or out_left:
        first, last = not words, body_left + out_left == 1
        if first or body_left == 0:
            is_out = not first
        else:                                                    # one OUT is kept for the very end
            is_out = out_left > 1 and int(rng.integers(0, body_left + out_left)) < out_left
        if is_out:
            if last:
                ka, ia = K_SLOT, n_slots - 1                     # the top slot, written by the first instruction, is read at the end
            else:
                ka, ia, _ = operand(out_kinds.pop() if out_kinds else None)
            words.append(instr_word(OP_OUT, int(rng.integers(0, 1 << 16)), ka, ia, int(rng.integers(0, 16)), int(rng.integers(0, 1 << 16))))
            out_left -= 1
            continue
        op, ka_kb = [OP_ADD, OP_SUB, OP_MUL][int(rng.integers(0, 3))], None
        if todo and (deg or K_SLOT not in todo[-1][1:]):
            op, *ka_kb = todo.pop()
        for _ in range(40):
            a = operand(ka_kb[0] if ka_kb else (leaves[int(rng.integers(0, len(leaves)))] if first else None))
            b = operand(ka_kb[1] if ka_kb else (leaves[int(rng.integers(0, len(leaves)))] if first else None))
            d = (a[2][0] + b[2][0], a[2][1] + b[2][1]) if op == OP_MUL else (max(a[2][0], b[2][0]), max(a[2][1], b[2][1]))
            if not bounded or (d[0] <= MAX_DEG[0] and d[1] <= MAX_DEG[1]):
                break
        else:
            op = OP_ADD if op == OP_MUL else op
            d = (max(a[2][0], b[2][0]), max(a[2][1], b[2][1]))
        dst = n_slots - 1 if first else _index(rng, n_slots)
        words.append(instr_word(op, dst, a[0], a[1], b[0], b[1]))
        deg[dst] = d
        body_left -= 1
    assert not todo and not out_kinds
    fills = list(fills) if fills is not None else [FILLS[int(rng.integers(0, 4))] for _ in lp]
    sparse = [(l, _sparse_column(rng, l, n_pub, f)) for l, f in zip(lp, fills)]
    table = []
    for l, ent in sparse:
        table.append(l | (len(ent) << 8))
        for pos, is_pub, v in ent:
            table += [pos | (int(is_pub) << 63), v]
    hdr = [MAGIC, width, 0, n_fixed, n_pub, 0, n_const, len(words), K, n_slots, 0, 1]
    blob = np.array(hdr + consts + words + table, dtype=np.uint64)
    shape = {"width": width, "n_pub": n_pub, "n_const": n_const, "n_slots": n_slots, "K": K, "lp": lp, "n_instr": len(words), "n_fixed": n_fixed,
             "sparse": sparse, "bounded": bounded}
    return blob, shape


# ---- the case set: (name, seed, shape).  tests/test_program_cases.py asserts what it covers (test_case_set_covers_the_grammar).
CASES = [
    ("cover", 101, dict(width=3, n_pub=5, n_const=7, n_slots=8, K=9, n_body=160, lps=(2,), cover=True)),
    ("one_slot_one_constraint", 102, dict(width=1, n_pub=3, n_const=0, n_slots=1, K=1, n_body=12)),
    ("slots32", 103, dict(width=4, n_pub=24, n_const=44, n_slots=32, K=6, n_body=220, lps=(0, 1, "n"))),
    ("many_constraints", 104, dict(width=2, n_pub=2, n_const=6, n_slots=8, K=140, n_body=150)),
    ("periods", 105, dict(width=3, n_pub=6, n_const=6, n_slots=8, K=5, n_body=60, lps=(0, 2, 2, 2, 1, 3, 1, "n"),
                          fills=("rand", "empty", "full", "pub", "rand", "full", "rand", "rand"))),
    ("no_publics", 106, dict(width=2, n_pub=0, n_const=3, n_slots=4, K=3, n_body=30, lps=(1,), fills=("full",))),
    ("bounded_a", 107, dict(width=3, n_pub=4, n_const=6, n_slots=8, K=5, n_body=40, lps=(0, 2, "n"), fills=("full", "rand", "rand"), bounded=True)),
    ("bounded_b", 108, dict(width=2, n_pub=3, n_const=6, n_slots=32, K=12, n_body=90, lps=(2, "n", 0), fills=("pub", "full", "rand"), bounded=True)),
    ("bounded_c", 109, dict(width=5, n_pub=2, n_const=2, n_slots=3, K=3, n_body=25, lps=("n", 0, 2), fills=("rand", "pub", "full"), bounded=True)),
]
BOUNDED = [c[0] for c in CASES if c[2].get("bounded")]


def case(name, logn=7):
    for n, seed, kw in CASES:
        if n == name:
            return gen(seed, logn, **kw)
    raise KeyError(name)


# ---- malformed blobs: one word of a good blob changed.  (class, blob) pairs; the classes are what every validating reader must refuse.
def malformed(blob, shape):
    """needs a blob with constants, publics, a non-OUT first instruction and a sparse column holding a constant and a public entry"""
    ins0 = HEADER_WORDS + shape["n_const"]
    tab0 = ins0 + shape["n_instr"]
    w0 = int(blob[ins0])
    assert w0 & 0xFF != OP_OUT and shape["n_const"] >= 1 and shape["n_pub"] >= 1

    def with_word(at, v):
        b = blob.copy()
        b[at] = v
        return b

    def operand_a(kind, idx):
        return with_word(ins0, (w0 & ~(0xFFFFF << 24)) | (kind << 24) | (idx << 28))

    def operand_b(kind, idx):
        return with_word(ins0, (w0 & ~(0xFFFFF << 44)) | (kind << 44) | (idx << 48))

    yield "opcode_0", with_word(ins0, w0 & ~0xFF)
    yield "opcode_5", with_word(ins0, (w0 & ~0xFF) | 5)
    yield "kind_7_a", operand_a(7, 0)
    yield "kind_7_b", operand_b(7, 0)
    lim = [shape["n_slots"], shape["width"], shape["width"], shape["n_fixed"], shape["n_pub"], shape["n_const"], 1]
    for kind in range(7):
        yield "index_at_limit_kind_%d" % kind, (operand_a if kind % 2 else operand_b)(kind, lim[kind])
    yield "dst_at_n_slots", with_word(ins0, (w0 & ~(0xFFFF << 8)) | (shape["n_slots"] << 8))
    yield "out_count_plus_1", with_word(8, shape["K"] + 1)
    yield "out_count_minus_1", with_word(8, shape["K"] - 1)
    yield "one_word_longer", np.concatenate([blob, np.zeros(1, dtype=np.uint64)])
    yield "one_word_shorter", blob[:-1].copy()
    for name, bad in malformed_sparse(blob, shape):
        yield name, bad


def malformed_sparse(blob, shape):
    """the classes that live in the sparse columns' table (what zp_fixed_columns reads too)"""
    at = HEADER_WORDS + shape["n_const"] + shape["n_instr"]
    const_at = pub_at = None
    for lp, ent in shape["sparse"]:
        for e, (pos, is_pub, v) in enumerate(ent):
            if is_pub and pub_at is None:
                pub_at = (at + 1 + 2 * e, lp)
            if not is_pub and const_at is None:
                const_at = (at + 1 + 2 * e, lp)
        at += 1 + 2 * len(ent)
    assert const_at and pub_at and at == len(blob)
    b = blob.copy()
    b[const_at[0]] = 1 << const_at[1]
    yield "entry_pos_at_period", b
    b = blob.copy()
    b[pub_at[0]] = (1 << 63) | (1 << pub_at[1])
    yield "public_entry_pos_at_period", b
    b = blob.copy()
    b[pub_at[0] + 1] = shape["n_pub"]
    yield "public_entry_index_at_n_pub", b
    b = blob.copy()
    b[const_at[0] + 1] = P
    yield "entry_value_p", b
