"""zp_poseidon_bn254_chains with ctx = NULL (the host path of the chain primitive, csrc/verify.hip) against the checker's width-17 permutation chained in
Python; its argument checks; and the transcript of every BN128-mode toy proof planned HERE as chain steps (a restatement of the block rule: values three
to an element and each absorb padded separately, a root one element, blocks of 16 that overwrite the rate, one bare permutation when nothing is queued,
48 values read out of a rate), run through the primitive and read back: the challenges and query indices are the checker's."""
import ctypes as C

import numpy as np
import pytest

import stark_verify_bn128_cases as BC
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
from oracle import oracle as O
from oracle import stark_verify as SV

P, R = SV.P, SV.R_BN254
ZP_ERR_ARG = -1


@pytest.fixture(scope="module")
def bn_tables():
    t = bn254_poseidon_params(17)
    O.p254_set(17, t[2], t[0], t[1])
    return t


def words(vals):
    return native.Prover._fr_words(vals)


def ints(a):
    return native.Prover._fr_ints(a)


def chained(chains):
    """chains: per chain a list of steps, a step None (bare) or 16 ints -> (blocks, absorb, first, want rates) with the checker's permutation"""
    blocks, absorb, first, want = [], [], [0], []
    for steps in chains:
        st = [0] * 17
        for blk in steps:
            if blk is not None:
                st = [st[0]] + list(blk)
            st = [int(v) for v in O.p254_perm([st], 17)[0]]
            blocks.append(list(blk) if blk is not None else [0] * 16)
            absorb.append(0 if blk is None else 1)
            want.append(st[1:])
        first.append(len(absorb))
    return blocks, absorb, first, want


def run(chains, bn_tables, prover=None):
    blocks, absorb, first, want = chained(chains)
    flat = words([v for b in blocks for v in b]).reshape(-1, 16, 4) if blocks else np.zeros((0, 16, 4), dtype=np.uint64)
    got = native.poseidon_bn254_chains(flat, absorb, first, prover=prover, bn_tables=bn_tables)
    assert got.shape == (len(absorb), 16, 4)
    for s in range(len(absorb)):
        assert ints(got[s]) == want[s], ("step", s)
    return got


def blocks_of(rng, n):
    return [[int.from_bytes(rng.bytes(32), "little") % R for _ in range(16)] for _ in range(n)]


def test_one_bare_permutation(bn_tables):
    got = run([[None]], bn_tables)
    assert ints(got[0]) == [int(v) for v in O.p254_perm([[0] * 17], 17)[0]][1:]


@pytest.mark.parametrize("n", [1, 2, 5])
def test_one_chain_absorbing_blocks(bn_tables, n):
    run([blocks_of(np.random.default_rng(40 + n), n)], bn_tables)


def test_absorbing_and_bare_steps_mixed(bn_tables):
    b = blocks_of(np.random.default_rng(50), 4)
    run([[b[0], None, None, b[1], b[2], None, b[3], [R - 1] * 16, [0] * 16]], bn_tables)


def test_four_chains_of_lengths_0_1_3_7(bn_tables):
    b = blocks_of(np.random.default_rng(60), 11)
    chains = [[], [b[0]], [None, b[1], b[2]], [b[3], b[4], None, b[5], b[6], None, b[7]]]
    got = run(chains, bn_tables)
    # a chain does not see its neighbours: each alone gives the same words
    at = 0
    for ch in chains:
        if ch:
            assert (run([ch], bn_tables) == got[at:at + len(ch)]).all()
        at += len(ch)


def test_argument_errors(bn_tables):
    lib = native.load_library()
    rc, mds, rp = bn_tables
    rcw, mw = words(rc), words([v for row in mds for v in row])
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)

    def call(blocks, absorb, first, nchains, rates=True, tables=True):
        bl = np.ascontiguousarray(blocks, dtype=np.uint64) if blocks is not None else None
        ab = np.ascontiguousarray(absorb, dtype=np.uint8) if absorb is not None else None
        fi = np.ascontiguousarray(first, dtype=np.uint32) if first is not None else None
        out = np.zeros(64 * max(1, len(absorb) if absorb is not None else 1), dtype=np.uint64)
        return lib.zp_poseidon_bn254_chains(None, bl.ctypes.data_as(u64p) if bl is not None else None, ab.ctypes.data_as(u8p) if ab is not None else None,
                                            fi.ctypes.data_as(u32p) if fi is not None else None, nchains, int(rp) if tables else 0,
                                            rcw.ctypes.data_as(u64p) if tables else None, mw.ctypes.data_as(u64p) if tables else None,
                                            out.ctypes.data_as(u64p) if rates else None)

    two = np.zeros((2, 16, 4), dtype=np.uint64)
    assert call(two, [1, 0], [0, 2], 1) == 0
    assert call(two, [1, 0], [0, 2], -1) == ZP_ERR_ARG                               # nchains < 0
    bad = two.copy()
    bad[1, 15] = words([R])[0]                                                       # a block element = r, in a bare step too
    assert call(bad, [1, 0], [0, 2], 1) == ZP_ERR_ARG
    bad[1, 15] = words([(1 << 256) - 1])[0]
    assert call(bad, [1, 0], [0, 2], 1) == ZP_ERR_ARG
    assert call(two, [1, 0], [1, 2], 1) == ZP_ERR_ARG                                # first does not start at 0
    assert call(two, [1, 0], [0, 2, 1], 2) == ZP_ERR_ARG                             # first decreases
    assert call(two, [1, 0], None, 1) == ZP_ERR_ARG                                  # null pointers with a non-empty call
    assert call(None, [1, 0], [0, 2], 1) == ZP_ERR_ARG
    assert call(two, None, [0, 2], 1) == ZP_ERR_ARG
    assert call(two, [1, 0], [0, 2], 1, rates=False) == ZP_ERR_ARG
    assert call(two, [1, 0], [0, 2], 1, tables=False) == ZP_ERR_ARG                  # ctx = NULL needs the caller's tables
    # chains of zero steps are legal and write nothing
    assert call(None, None, [0, 0, 0], 2, rates=False) == 0
    assert call(None, None, None, 0, rates=False) == 0


# ---- a proof's transcript as chain steps, planned here from the protocol (stark/prover.py; the checker's order: oracle/stark_verify.py verify)
class Plan:
    def __init__(self):
        self.queue, self.steps, self.reads, self.fresh = [], [], [], False

    def absorb(self, vals):
        v = [int(x) % P for x in vals]
        v += [0] * (-len(v) % 3)                                  # each absorb padded separately
        self.queue += [v[i] | (v[i + 1] << 64) | (v[i + 2] << 128) for i in range(0, len(v), 3)]
        self.fresh = False

    def absorb_root(self, root):
        self.queue.append(int(root[0]))
        self.fresh = False

    def squeeze(self, n):
        """returns where the n values will stand: (step, position among the 48 values of its rate)"""
        out = []
        for _ in range(n):
            if self.queue or not self.fresh or self.pos == 48:
                if not self.queue:
                    self.steps.append(None)
                for off in range(0, len(self.queue), 16):
                    blk = self.queue[off:off + 16]
                    self.steps.append(blk + [0] * (16 - len(blk)))
                self.queue, self.fresh, self.pos = [], True, 0
            out.append((len(self.steps) - 1, self.pos))
            self.pos += 1
        return out


def plan_of(case, tables):
    pr, ex = case.proof, case.expect
    prog = case.program
    W, W2, n_s2 = int(prog[1]), int(prog[2]), int(prog[10])
    pubs = pr["publics"]
    dg = [int(d) % P for d in _digest_words(prog)]
    head = [ex["logn"], ex["logb"], W, W2, ex["fri_logf"], ex["fri_final_log"], ex["n_queries"], ex["pow_bits"], ex["root32"], ex["shift"]] + dg + [len(pubs)]
    t, at = Plan(), {}
    if len(pubs) <= 64:
        t.absorb(head + pubs)
    else:
        t.absorb(head)
        t.absorb_root(SV.publics_digest(pubs, *tables, True))
    t.absorb_root(pr["roots"]["trace"])
    if n_s2:
        at["chal"] = t.squeeze(3)
        t.absorb_root(pr["roots"]["stage2"])
    at["alpha"] = t.squeeze(3)
    t.absorb_root(pr["roots"]["quotient"])
    at["zeta"] = t.squeeze(3)
    t.absorb([v for row in pr["evals"]["z"] for v in row])
    t.absorb([v for row in pr["evals"]["zw"] for v in row])
    at["gamma"] = t.squeeze(3)
    at["betas"] = []
    for root in pr["fri"]["roots"]:
        t.absorb_root(root)
        at["betas"].append(t.squeeze(3))
    for c in range(3):
        t.absorb(pr["fri"]["final"][c])
    at["indices"] = t.squeeze(ex["n_queries"])
    return t.steps, at


def _digest_words(program):
    import hashlib
    d = hashlib.sha256(np.ascontiguousarray(program, dtype=np.uint64).tobytes()).digest()
    return [int.from_bytes(d[8 * i:8 * i + 8], "little") for i in range(4)]


_cases = {}


def case_of(name, tables, bn_tables):
    if name not in _cases:
        cpu = BC.cpu_backend(tables, bn_tables)
        _cases[name] = BC.make_vair_case(cpu, tables) if name == "vair" else BC.make_case(name, cpu)
    return _cases[name]


@pytest.mark.parametrize("name", BC.NAMES)
def test_transcripts_replayed_through_the_primitive_give_the_checkers_challenges(tables, bn_tables, name):
    case = case_of(name, tables, bn_tables)
    want = SV.verify(case.proof, case.program, *tables, case.expect, bn_tables, header_only=True)
    steps, at = plan_of(case, tables)
    assert name != "vair" or len(case.proof["publics"]) > 64
    blocks = words([v for s in steps for v in (s if s is not None else [0] * 16)]).reshape(-1, 16, 4)
    rates = native.poseidon_bn254_chains(blocks, [0 if s is None else 1 for s in steps], [0, len(steps)], bn_tables=bn_tables)

    def read(where):
        out = []
        for step, pos in where:
            e = ints(rates[step])[pos // 3]
            out.append(((e >> (64 * (pos % 3))) & 0xFFFFFFFFFFFFFFFF) % P)
        return out

    M = 1 << (case.expect["logn"] + case.expect["logb"])
    assert read(at["zeta"]) == [int(v) for v in want["zeta"]]
    assert read(at["gamma"]) == [int(v) for v in want["gamma"]]
    assert [read(b) for b in at["betas"]] == [[int(v) for v in b] for b in want["betas"]]
    assert [v & (M - 1) for v in read(at["indices"])] == [int(v) for v in want["indices"]]
