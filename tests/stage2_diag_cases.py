"""What tests/test_stage2_diag_host.py and tests/test_gpu_stage2_diag.py share: the expected records of zp_stark_diagnose_stage2 and the case set.
TEST INFRASTRUCTURE.

The expectation follows include/zeth_prover.h's definitions with collections.Counter: lhs(v) = occurrences of v in column a, rhs(v) = occurrences
in b (permutation) or the sum of m over the rows with t = v, taken % P (lookup); v is unbalanced when they differ.  Blobs are those of
WC.honest_case("perm") (one permutation {0, 1}) and ("chunk16") (a permutation, then a lookup); the call evaluates no constraint, so the traces
are built freely on them."""
import functools
from collections import Counter

import numpy as np

import witness_cases as WC
from oracle.air_program import Program

P = WC.P
NONE = WC.NONE
HOLDS, FAILS, NONCANONICAL = 0, 1, 2
WORDS = 12
LOGNS = (1, 5, 6, 9, 12)        # under one wave, one wave, one workgroup and a bit, several, many


def expected(blob, trace, logn):
    """[record of 12 ints] per stage-2 argument -- what zp_stark_diagnose_stage2 must write, word for word"""
    prog = Program(blob)
    tr = np.asarray(trace, dtype=np.uint64).reshape(prog.width, 1 << logn)
    if (tr >= np.uint64(P)).any():
        return [[NONCANONICAL, s["kind"], 0, NONE, NONE, 0, 0, NONE, NONE, 0, 0, 0] for s in prog.stage2]
    out = []
    for s in prog.stage2:
        a, b = [int(v) for v in tr[s["a"]]], [int(v) for v in tr[s["b"]]]
        m = [int(v) for v in tr[s["m"]]] if s["kind"] == 2 else [1] * len(b)
        lhs, rhs = Counter(a), Counter()
        for v, w in zip(b, m):
            rhs[v] = (rhs[v] + w) % P
        bad = {v for v in set(lhs) | set(rhs) if lhs[v] != rhs[v]}
        side = lambda col: next(([r, v, lhs[v], rhs[v]] for r, v in enumerate(col) if v in bad), [NONE, NONE, 0, 0])
        out.append([FAILS if bad else HOLDS, s["kind"], len(bad)] + side(a) + side(b) + [sum(lhs[v] for v in bad)])
    return out


def arguments(blob):
    return Program(blob).stage2


def with_columns(name, logn, cols):
    """(blob, trace): the honest trace of a built-in AIR with the columns of `cols` {index: values} replaced"""
    _, blob, tr, _ = WC.honest_case(name, logn)
    t = np.array(tr, dtype=np.uint64)
    for c, vals in cols.items():
        t[c] = np.array([int(v) for v in vals], dtype=np.uint64)
    return blob, t


def perm_case(logn, a, b):
    return with_columns("perm", logn, {0: a, 1: b})


def lookup_case(logn, a, t, m):
    """chunk16 with the lookup's columns set; the permutation's other column follows a, so only the lookup is in question"""
    blob = WC.honest_case("chunk16", logn)[1]
    perm, look = arguments(blob)
    assert (perm["kind"], look["kind"]) == (1, 2) and perm["a"] == look["a"]
    return with_columns("chunk16", logn, {look["a"]: a, perm["b"]: a, look["b"]: t, look["m"]: m})


def collision_values(kind, n):
    """n distinct canonical values built to collide under a simple hash (low bits, high bits, a shift, a fold)"""
    if kind == "hi32":
        return [i << 32 for i in range(n)]
    if kind.startswith("shift"):
        return [i << int(kind[5:]) for i in range(n)]
    if kind == "top":
        return [P - 1 - i for i in range(n)]
    assert kind == "ends"
    return [(0, P - 1)[i & 1] for i in range(n)]      # two values only


COLLISIONS = ("hi32", "shift8", "shift16", "shift20", "shift44", "top", "ends")


@functools.lru_cache(maxsize=None)
def case(name, logn):
    """(blob, trace, edited row or None)"""
    N = 1 << logn
    if name in ("honest_perm", "honest_chunk16"):
        _, blob, tr, _ = WC.honest_case(name[7:], logn)
        return blob, np.array(tr, dtype=np.uint64), None
    if name == "broken_perm":
        blob, t, _ = WC.broken_perm(logn)
        return blob, t, 3 % N
    if name == "broken_lookup":
        blob, t, _ = WC.broken_lookup(logn)
        return blob, t, 5 % N
    if name == "multiplicity":        # one m[i] + 1, one m[k] - 1 on table rows that are hit
        _, blob, tr, _ = WC.honest_case("chunk16", logn)
        look = arguments(blob)[1]
        t = np.array(tr, dtype=np.uint64)
        hit = [int(i) for i in np.nonzero(t[look["m"]] != 0)[0]]
        i, k = hit[0], hit[-1]
        assert i != k and int(t[look["b"], i]) != int(t[look["b"], k])
        t[look["m"], i] += np.uint64(1)
        t[look["m"], k] -= np.uint64(1)
        return blob, t, i
    if name in ("m_mod_p", "m_mod_p_off"):      # value 7 hit c times, stored in two table rows with m = p - 1 and c + 1 (or c: rhs = c - 1)
        c = N // 2
        a = [7] * c + [9] * (N - c)
        t = [7, 7] + [9] * (N - 2)
        m = [P - 1, c + 1 if name == "m_mod_p" else c, N - c] + [0] * (N - 3)
        return lookup_case(logn, a, t, m) + (None,)
    if name in ("one_value", "one_value_short"):      # a whole column of one value against one table row
        t = [5] + [6 + i for i in range(N - 1)]
        m = [N if name == "one_value" else N - 1] + [0] * (N - 1)
        return lookup_case(logn, [5] * N, t, m) + (None,)
    if name == "disjoint":            # 2 N distinct keys: the table's maximum load
        return perm_case(logn, range(N), range(N, 2 * N)) + (None,)
    if name == "noncanonical":        # one word >= p in a column no argument reads
        _, blob, tr, _ = WC.honest_case("chunk16", logn)
        t = np.array(tr, dtype=np.uint64)
        assert all(0 not in (s["a"], s["b"]) + ((s["m"],) if s["kind"] == 2 else ()) for s in arguments(blob))
        t[0, N - 1] = np.uint64(P)
        return blob, t, None
    kind, broken = name.split(":")[1], name.endswith(":broken")
    vals = collision_values(kind, N)
    b = vals[::-1]
    if broken:                        # b takes its neighbour's value: two unbalanced values
        b[N // 2] = b[N // 2 - 1]
    return perm_case(logn, vals, b) + (None,)


CASES = ["honest_perm", "honest_chunk16", "broken_perm", "broken_lookup", "disjoint", "noncanonical"]
CASES += ["collide:%s:%s" % (k, w) for k in COLLISIONS for w in ("whole", "broken")]
LOOKUP_CASES = ["multiplicity", "m_mod_p", "m_mod_p_off", "one_value", "one_value_short"]      # need N >= 4


def all_cases():
    """(name, logn) of every case: each at LOGNS (the lookup constructions from 2^5 rows on), and one of 2^16 rows"""
    out = [(n, l) for n in CASES for l in LOGNS] + [(n, l) for n in LOOKUP_CASES for l in LOGNS if l >= 5]
    return out + [("disjoint", 16)]
