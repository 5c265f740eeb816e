"""Shared by tests/test_r1cs_cases.py and tests/test_gpu_r1cs_device.py: seeded small circuits at the seams of the device R1CS evaluator
(csrc/r1cs.hip: zp_r1cs_eval_device), built with service/r1cs.py (Circuit, poseidon_template(17)) and service/arith.py (Builder).

One generator (`build`) makes every shape from (structure seed, gadget instances per wave -- three waves --, arithmetic instances, explicit
definitions, plain explicit rows, public inputs):
  values      caller-set field elements half from the corners {0, 1, 2, r-1, r-2, 2^253, 2^64-1, 2^64}, half uniform; coefficients from
              {1, r-1, 2, random}; arithmetic inputs from {0, 1, p-1, 2^64-1, random 64-bit}
  arithmetic  one template: an e3_mul of its two input triples, an e3_inv of the first (the inverse of zero: no witness) and a product of two
              combinations with coefficients other than 1
  gadgets     the inputs of a wave-k instance are caller-set wires and outputs of earlier waves (one output of wave k-1 at least)
  explicit    a CHAIN of definitions (each reads the one before it, earlier ones, gadget outputs, caller wires), the last n_pub of them
              defining the public wires (wire 1 by the last row); plain rows A.B = C that hold, interleaved -- C holds a caller-set wire of
              the row's own whose value the generator computes
PRECONDITION: a definition precedes every row that reads the wire it defines, and no gadget reads a defined wire.  The host evaluator walks
the explicit rows in order and the device evaluator runs all definitions before all rows; an ill-ordered circuit is out of scope.

`Case.tags` names the wires and rows the refusal tests aim at (a caller wire read only by a wave-1 gadget, only by a plain row, only by the
definition in the middle of the chain, by nobody ...)."""
import copy
import functools
import random

import numpy as np

from eigen_zeth_amd import native
from eigen_zeth_amd.service import arith as AR
from eigen_zeth_amd.service import r1cs as R1

R, P = R1.R, AR.P
W64 = (1 << 64) - 1
CORNERS = (0, 1, 2, R - 1, R - 2, 1 << 253, W64, 1 << 64)
TC = 613                                 # rows (= internal wires) of the width-17 gadget

# name -> (structure seed, instances per wave, arithmetic instances, definitions, plain rows, public inputs, arithmetic wires read from outside)
SHAPES = {
    "S1": (101, (1, 0, 0), 0, 9, 0, 1, False),        # one of a gadget block's three slots live
    "S2": (102, (7, 4, 1), 3, 9, 8, 1, False),        # no wave a multiple of 3; waves start at instances 7 and 11
    "S3": (103, (64, 5, 2), 257, 40, 300, 1, False),  # 256 + 1 arithmetic instances, a second block of explicit rows, a 40-long chain
    "S4": (104, (7, 4, 1), 3, 9, 8, 1, True),         # a definition and a gadget input that read an arithmetic instance's output
    "S5": (105, (0, 0, 0), 0, 2, 0, 2, False),        # no gadget instance, two rows, two public inputs
}
WAVE_BOUNDS = {"S1": [0, 1], "S2": [0, 7, 11, 12], "S3": [0, 64, 69, 71], "S4": [0, 7, 11, 12], "S5": [0, 0]}
LOGM = {"S1": 10, "S2": 14, "S3": 18, "S4": 14, "S5": 2}


@functools.lru_cache(maxsize=None)
def arith_template():
    """inputs a[3], c[3] (64-bit values); internal: a c and 1 / a in F_p^3, and one product of two combinations of the inputs.  Returns (template, local wires of the reduced product)"""
    b = AR.Builder()
    a = [b.inp(W64) for _ in range(3)]
    c = [b.inp(W64) for _ in range(3)]
    A, C = b.e3(a), b.e3(c)
    prod = b.e3_mul(A, C)
    b.e3_inv(A)
    # every other row's non-unit combination is an identity whose value is 0: this product of two combinations is the row where a template
    # coefficient meets a non-zero value (the device's coefficient arithmetic would otherwise go unseen)
    b.mul(A[0] + A[1] * 3 + 5, C[0] + C[2] * (P - 1) + 1, "product of combinations")
    return b.template(), [next(iter(x.t)) for x in prod]


class Case:
    """circuit: the R1.Circuit; blob: its packed form; vals: {wire: value} of the caller-set wires (wire 0 included); tags: see the module"""

    def __init__(self, name, circuit, blob, vals, tags):
        self.name, self.circuit, self.blob, self.vals, self.tags = name, circuit, blob, vals, tags
        self.n_wires, self.n_cons, self.logm, self.n_pub = int(blob[1]), int(blob[2]), int(blob[3]), int(blob[9])

    def arrays(self, vals=None):
        """(witness u64[n_wires][4], mask) for native.r1cs_eval"""
        vals = self.vals if vals is None else vals
        ids = np.array(sorted(vals), dtype=np.int64)
        w = np.zeros((self.n_wires, 4), dtype=np.uint64)
        mask = np.zeros(self.n_wires, dtype=np.uint8)
        w[ids] = native.fr_words([vals[int(k)] for k in ids])
        mask[ids] = 1
        return w, mask

    def set_lists(self, vals=None, order_seed=7):
        """(set_idx u64[n], set_val u64[n][4]) for zp_r1cs_eval_device, in a shuffled order (the scatter kernel's input is a list, not a mask)"""
        vals = self.vals if vals is None else vals
        ids = sorted(vals)
        random.Random(order_seed).shuffle(ids)
        return np.array(ids, dtype=np.uint64), native.fr_words([vals[k] for k in ids])

    def without(self, wire):
        return {k: v for k, v in self.vals.items() if k != wire}

    def with_value(self, wire, value):
        out = dict(self.vals)
        out[wire] = value % R
        return out


def _field_value(rnd):
    return rnd.choice(CORNERS) if rnd.random() < 0.5 else rnd.randrange(R)


def _coef(rnd):
    return rnd.choice((1, R - 1, 2, rnd.randrange(1, R)))


def _arith_value(rnd):
    return rnd.choice((0, 1, P - 1, W64, rnd.randrange(1 << 64)))


def _lc(rnd, wires, n_lo, n_hi, must=()):
    """a combination of n_lo..n_hi distinct wires of `wires` (and every wire of `must`) with coefficients from _coef"""
    n = min(rnd.randint(n_lo, n_hi), len(wires))
    out = {k: _coef(rnd) for k in rnd.sample(wires, n)}
    for k in must:
        out[k] = _coef(rnd)
    return out


def build(name, seed, waves, n_arith, n_defs, n_plain, n_pub, arith_links, value_seed=None):
    rs = random.Random(seed)                                     # structure
    rv = random.Random(seed * 7919 + 1 if value_seed is None else value_seed)   # values
    assert len(waves) == 3 and n_defs >= n_pub
    c = R1.Circuit(R1.poseidon_template(17), n_pub=n_pub)
    tags = {}
    pool = c.new_wires(24)                                       # caller-set wires anybody may read
    field_wires = list(pool)
    for tag, wanted in (("only_wave1", waves[1] > 0), ("only_plain", n_plain > 0), ("only_mid_def", n_defs >= 3), ("unread", True)):
        if wanted:
            tags[tag] = c.new_wire()
            field_wires.append(tags[tag])
    # ---- arithmetic instances
    arith_inputs, arith_out = [], []
    if n_arith:
        T, prod = arith_template()
        h = c.add_arith_template(T)
        for _ in range(n_arith):
            ins = c.new_wires(T.n_in)
            g = c.add_arith(h, ins)
            arith_inputs.append(ins)
            arith_out.append([g(k) for k in prod])
        tags["arith_input"] = arith_inputs[0][4]
        tags["arith_rows"] = len(T.rows)
        tags["arith_n_int"] = T.n_int
    # ---- gadget waves
    outs = [[], [], []]
    for k in range(3):
        earlier = [o for prev in outs[:k] for o in prev]
        for i in range(waves[k]):
            ins = [rs.choice(pool + earlier) for _ in range(17)]
            if k:
                ins[rs.randrange(1, 17)] = rs.choice(outs[k - 1])   # what puts the instance into wave k
            if k == 1 and i == waves[1] - 1:
                ins[0] = tags["only_wave1"]
            if arith_links and k == 0 and i == 2:
                ins[3] = arith_out[1][2]                         # a gadget input that is an arithmetic instance's internal wire
                tags["gadget_reads_arith"] = (i, arith_out[1][2])
            outs[k].append(c.add_instance(ins))
    if waves[0]:
        tags["wave0_input"] = next(w for w in c.instances[0][0] if w in pool)
    gadget_outs = [o for ws in outs for o in ws]
    # ---- explicit rows: definitions (a chain) and plain rows, interleaved; every plain row follows the definitions it reads
    readable = pool + gadget_outs
    defined, plain_z = [], []                                    # plain_z[q]: the row's own caller-set wire, None for a definition
    order = ["def"] * n_defs
    for _ in range(n_plain):
        order.insert(rs.randrange(1, len(order)), "plain")       # never first, never last: the last row defines public wire 1
    k_def = 0
    for what in order:
        src = readable + defined
        if what == "plain":
            z = c.new_wire()
            must = [tags["only_plain"]] if "plain_row" not in tags else []
            A, B = _lc(rs, src, 0 if must else 1, 4, must), _lc(rs, src, 1, 3)
            C = _lc(rs, src, 0, 2)
            C[z] = 1
            if "plain_row" not in tags:
                tags["plain_row"] = (len(c.extras), z)
            c.add_constraint(A, B, C)
            plain_z.append(z)
            continue
        left = n_defs - k_def                                    # the last n_pub definitions define the public wires n_pub .. 1
        d = left if left <= n_pub else c.new_wire()
        must_a = [defined[-1]] if defined else []
        if k_def == n_defs // 2 and "only_mid_def" in tags:
            must_a.append(tags["only_mid_def"])
            tags["mid_def"] = (len(c.extras), d)
        must_b = []
        if arith_links and k_def == 1:
            must_b.append(arith_out[2][0])                       # a definition that reads an arithmetic instance's internal wire
            tags["def_reads_arith"] = (len(c.extras), arith_out[2][0])
        A, B = _lc(rs, src, 1, 3, must_a), _lc(rs, src, 1, 3, must_b)
        C = _lc(rs, [w for w in src if w != d], 0, 2)
        C[d] = 1
        c.add_constraint(A, B, C, defines=d)
        plain_z.append(None)
        defined.append(d)
        k_def += 1
    tags["defined"] = defined
    tags["plain_z"] = [z for z in plain_z if z is not None]
    blob = c.pack()
    # ---- values
    vals = {0: 1}
    for k in field_wires:
        vals[k] = _field_value(rv)
    for ins in arith_inputs:
        for k in ins:
            vals[k] = _arith_value(rv)
        if all(vals[k] % P == 0 for k in ins[:3]):
            vals[ins[0]] = 1                                     # zero has no inverse: kept for the refusal tests
    # the plain rows' own wires: what the row gives when it is read as their definition (a sibling circuit that differs in nothing else)
    sib = copy.copy(c)
    sib.extras = [(A, B, C, z if z is not None else d) for (A, B, C, d), z in zip(c.extras, plain_z)]
    full = sib.complete(vals)
    for z in tags["plain_z"]:
        vals[z] = full[z]
    tags["arith_inputs"] = arith_inputs
    return Case(name, c, blob, vals, tags)


@functools.lru_cache(maxsize=None)
def case(name, value_seed=None):
    seed, waves, n_arith, n_defs, n_plain, n_pub, links = SHAPES[name]
    return build(name, seed, waves, n_arith, n_defs, n_plain, n_pub, links, value_seed)


def host_refusal(cs, vals):
    """(code, bad) of zp_r1cs_eval for an assignment it refuses"""
    try:
        native.r1cs_eval(cs.blob, *cs.arrays(vals))
    except ValueError as e:
        return -20, int(str(e).split("constraint ")[1].split(")")[0])
    except native.ZpError as e:
        return e.code, e.bad
    raise AssertionError("accepted")


def faults(cs):
    """name -> the assignment with one fault (one per refusal test, host and device)"""
    t = cs.tags
    ref = cs.circuit.complete(cs.vals)
    out = {"unset: " + k: cs.without(t[k]) for k in ("wave0_input", "only_wave1", "only_plain", "only_mid_def", "arith_input", "unread")}
    d = t["defined"][len(t["defined"]) // 2 - 1]
    out["violated: a defined wire set off by one"] = cs.with_value(d, ref[d] + 1)
    out["violated: a plain row"] = cs.with_value(t["plain_row"][1], ref[t["plain_row"][1]] + 1)
    z = ref[t["plain_row"][1]]                                   # ... and off in the top one of the device's nine 29-bit limbs only (bits 232 up)
    out["violated: a plain row, in the top limb only"] = cs.with_value(t["plain_row"][1], next(z ^ (1 << b) for b in range(240, 231, -1) if z ^ (1 << b) < R))
    zero = dict(cs.vals)
    for k in t["arith_inputs"][1][:3]:
        zero[k] = 0
    out["violated: e3_inv of zero in the second arithmetic instance"] = zero
    return out
