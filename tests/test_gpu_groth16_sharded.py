"""The Groth16 wrap over the ranks of a communicator: zp_msm_bn254_sharded / _g2_sharded and zp_groth16_prove_sharded.  Every rank holds its
slice of the points (k = ceil(n / world), rank r owns [r k, min((r + 1) k, n))), the partial sums travel in one all-gather and are added in
rank order, so every rank's result must equal, word for word, the one-ctx call on the whole input.  The multi-rank cases run as thread-ranks
on one GPU (zp_comm_group_create / zp_comm_create_local): a rehearsal of the multi-GPU path, not a speed-up."""
import json
import random
import threading

import numpy as np
import pytest

from eigen_zeth_amd import native
from eigen_zeth_amd.service import groth16 as G16
from eigen_zeth_amd.service import wrap_circuit as WC
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR
from eigen_zeth_amd.stark.backend_hip import HipBackend
from oracle import groth16_verify as GV
from oracle import naive_bn254 as B

pytestmark = pytest.mark.gpu


def run_ranks(G, fn, timeout_ms=None):
    """fn(rank, prover, comm) on G thread-ranks on GPU 0 (one Prover and one local Comm each) -> (results, errors) by rank"""
    group = native.CommGroup(G)
    out, err = [None] * G, [None] * G

    def body(r):
        p, c = None, None
        try:
            p = native.Prover(0)
            c = native.Comm(p, r, G, group=group)
            if timeout_ms is not None:
                c.set_timeout_ms(timeout_ms)
            out[r] = fn(r, p, c)
        except BaseException as e:      # noqa: every rank's outcome is returned
            err[r] = e
        finally:
            if c is not None:
                c.close()
            if p is not None:
                p.close()
    ts = [threading.Thread(target=body, args=(r,)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    group.close()
    assert not any(t.is_alive() for t in ts), "a rank is stuck in a collective"
    return out, err


def upload_u32(p, arr):
    """a device copy of a uint32 array (None when it is empty: an empty slice passes NULL)"""
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    if arr.size == 0:
        return None
    d = p.alloc((arr.nbytes + 7) // 8)
    p._chk(p.lib.zp_h2d(p.ctx, d.ptr, arr.ctypes.data, arr.nbytes))
    return d


def msm_over_ranks(G, pts, scs, g2=False):
    """zp_msm_bn254(_g2)_sharded over G thread-ranks; every rank's words"""
    n = pts.shape[0]

    def fn(r, p, c):
        first, count = c.my_range(n)
        d_p, d_s = upload_u32(p, pts[first:first + count]), upload_u32(p, scs[first:first + count])
        try:
            return c.msm_bn254_sharded(d_p, d_s, n, g2=g2)
        finally:
            for d in (d_p, d_s):
                if d is not None:
                    d.free()
    out, err = run_ranks(G, fn)
    for e in err:
        if e is not None:
            raise e
    return out


def one_ctx(prover, pts, scs, g2=False):
    n = pts.shape[0]
    d_p, d_s = upload_u32(prover, pts), upload_u32(prover, scs)
    out = np.zeros(32 if g2 else 16, dtype=np.uint32)
    fn = prover.lib.zp_msm_bn254_g2 if g2 else prover.lib.zp_msm_bn254
    try:
        prover._chk(fn(prover.ctx, d_p.ptr, d_s.ptr, n, out.ctypes.data_as(native.C.POINTER(native.C.c_uint32))))
    finally:
        d_p.free()
        d_s.free()
    return out


def words_g1(p):
    return G16._g1_words(p)


def words_g2(p):
    return G16._g2_words(p)


@pytest.fixture(scope="module")
def g1_table():
    """16 points k_j G with their discrete logs: the oracle's sum of any MSM over them is ONE scalar multiplication of G (linearity)"""
    rnd = random.Random(0x5A4D)
    ks = [rnd.randrange(1, B.R) for _ in range(16)]
    return ks, np.stack([words_g1(B.mul(B.G, k)) for k in ks])


@pytest.fixture(scope="module")
def g2_table():
    rnd = random.Random(0x5A4E)
    ks = [rnd.randrange(1, B.R) for _ in range(8)]
    return ks, np.stack([words_g2(B.mul_g2(B.G2, k)) for k in ks])


def draw(table, n, seed):
    ks, tw = table
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(ks), size=n)
    scs = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    return idx, np.ascontiguousarray(tw[idx]), scs


def oracle_g1(ks, idx, scs):
    total = sum(ks[int(i)] * sum(int(s[k]) << (32 * k) for k in range(8)) for i, s in zip(idx, scs)) % B.R
    return words_g1(B.mul(B.G, total) if total else None)


def oracle_g2(ks, idx, scs):
    total = sum(ks[int(i)] * sum(int(s[k]) << (32 * k) for k in range(8)) for i, s in zip(idx, scs)) % B.R
    return words_g2(B.mul_g2(B.G2, total) if total else None)


@pytest.mark.parametrize("n", [1, 3, 7, 1000, (1 << 16) + 3, 1 << 20])
def test_g1_msm_over_ranks_equals_the_one_ctx_msm(prover, g1_table, n):
    """n < G leaves ranks with empty slices (they add infinity); every rank returns the one-ctx words, and the oracle's for n <= 1000"""
    idx, pts, scs = draw(g1_table, n, 1000 + n)
    want = one_ctx(prover, pts, scs)
    if n <= 1000:
        assert (want == oracle_g1(g1_table[0], idx, scs)).all()
    for G in (2, 4, 8):
        for got in msm_over_ranks(G, pts, scs):
            assert (got == want).all(), "G = %d" % G


def test_g1_msm_over_ranks_edge_cases(prover, g1_table):
    ks, tw = g1_table
    p = B.mul(B.G, ks[0])
    # P in rank 0's slice, -P in rank 1's: the partial sums cancel across the rank boundary
    pts = np.stack([words_g1(p), words_g1((p[0], B.Q - p[1]))])
    scs = np.zeros((2, 8), dtype=np.uint32)
    scs[:, 0] = 5
    for got in msm_over_ranks(2, pts, scs):
        assert not got.any()
    # every input at infinity
    pts = np.zeros((100, 16), dtype=np.uint32)
    scs = np.random.default_rng(9).integers(0, 1 << 32, size=(100, 8), dtype=np.uint64).astype(np.uint32)
    for got in msm_over_ranks(4, pts, scs):
        assert not got.any()
    # skewed scalars on ONE rank only (all ones in rank 1's slice of 4: its buckets are heavy, the others' are not)
    n = 3000
    idx, pts, scs = draw(g1_table, n, 77)
    first, count = 750, 750
    scs[first:first + count] = 0
    scs[first:first + count, 0] = 1
    want = one_ctx(prover, pts, scs)
    assert (want == oracle_g1(ks, idx, scs)).all()
    for got in msm_over_ranks(4, pts, scs):
        assert (got == want).all()


@pytest.mark.parametrize("n", [1, 3, 7, 1000, (1 << 16) + 3])
def test_g2_msm_over_ranks_equals_the_one_ctx_msm(prover, g2_table, n):
    idx, pts, scs = draw(g2_table, n, 2000 + n)
    want = one_ctx(prover, pts, scs, g2=True)
    if n <= 1000:
        assert (want == oracle_g2(g2_table[0], idx, scs)).all()
    for G in (2, 4, 8):
        for got in msm_over_ranks(G, pts, scs, g2=True):
            assert (got == want).all(), "G = %d" % G


def test_g2_msm_over_ranks_edge_cases(prover, g2_table):
    ks, tw = g2_table
    p = B.mul_g2(B.G2, ks[1])
    neg = (p[0], ((B.Q - p[1][0]) % B.Q, (B.Q - p[1][1]) % B.Q))
    pts = np.stack([words_g2(p), words_g2(neg)])
    scs = np.zeros((2, 8), dtype=np.uint32)
    scs[:, 0] = 3
    for got in msm_over_ranks(2, pts, scs, g2=True):
        assert not got.any()
    pts = np.zeros((50, 32), dtype=np.uint32)
    for got in msm_over_ranks(4, pts, scs[:1].repeat(50, axis=0), g2=True):
        assert not got.any()
    n = 1400
    idx, pts, scs = draw(g2_table, n, 78)
    scs[350:700] = 0
    scs[350:700, 0] = 1                                      # rank 1 of 4: heavy buckets
    want = one_ctx(prover, pts, scs, g2=True)
    assert (want == oracle_g2(ks, idx, scs)).all()
    for got in msm_over_ranks(4, pts, scs, g2=True):
        assert (got == want).all()


def test_large_distinct_g1_msm_over_eight_ranks(prover):
    """2^24 distinct points (zp_synth_g1_points) over 8 ranks = the one-ctx MSM"""
    n = 1 << 24
    pts = native.synth_g1_points(n)
    scs = np.random.default_rng(24).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    want = one_ctx(prover, pts, scs)
    for got in msm_over_ranks(8, pts, scs):
        assert (got == want).all()


# ---- Groth16 over the ranks, on the wrap circuit of a small BN128-mode STARK (built as tests/test_gpu_wrap.py builds it)

RAND = (0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321)


@pytest.fixture(scope="module")
def wrap():
    hip = HipBackend(0, hash_mode="bn128")
    air = AIR.get_air("wide8")
    tr, pub = native.synth_trace(air.trace_kind, 8, air.width, 5)
    params = PR.StarkParams(8, 2, 3, 3, 6, pow_bits=0, hash="bn128")
    json.loads(hip.prove_native(air, tr, pub, params))
    wc = WC.wrap_circuit(WC.Layout.of_air(air, params))
    set_idx, set_val = native.wrap_assign(wc.script, hip.stark_openings(), 12345)
    key = G16.Key(wc.blob)
    ref = G16.prove(key, set_idx, set_val, hip, RAND)             # zp_groth16_prove on one ctx, the whole key
    yield hip, wc, key, set_idx, set_val, ref
    hip.p.close()


@pytest.mark.parametrize("G", [2, 4])
def test_groth16_over_ranks_equals_the_one_ctx_proof(wrap, G):
    hip, wc, key, set_idx, set_val, (p_ref, pub_ref, _) = wrap
    provers = [native.Prover(0) for _ in range(G)]
    try:
        proof, pub, ms = G16.prove_sharded(key, set_idx, set_val, provers, RAND)      # asserts that every rank returned the same words
        assert proof == p_ref and pub == pub_ref
        assert G16.proof_to_json(proof) == G16.proof_to_json(p_ref)
        assert GV.verify(key.vk, proof, pub)
        assert len(ms) == 8
        # the slices: rank r holds ceil(n / G) points of each array (the tail fewer), so the key's memory per rank drops to 1 / G
        sl = key.load_slices(provers)
        n_u = int(key.u.shape[0]) + 2
        assert sum(s["u1x"].n * 8 // 64 for s in sl if s["u1x"] is not None) >= n_u
        assert max(s["u1x"].n for s in sl) * 8 // 64 <= -(-n_u // G) + 1
    finally:
        key._slices = None
        for q in provers:
            q.close()


def test_groth16_over_ranks_refuses_a_false_assignment_on_every_rank(wrap):
    hip, wc, key, set_idx, set_val, _ = wrap
    bad = set_val.copy()
    bad[int(np.flatnonzero(set_idx == np.uint64(wc.q[1]["trees"][2]["levels"][0]["sib"][5]))[0]), 0] ^= np.uint64(1)      # one digest of one path
    provers = [native.Prover(0) for _ in range(2)]
    try:
        slices = key.load_slices(provers)
        d1 = G16._g1_words(B.mul(B.G, key.toxic["delta"]))
        errs = [None, None]

        def body(r):
            c = native.Comm(provers[r], r, 2, group=group)
            try:
                c.set_timeout_ms(5000)
                c.groth16_prove_sharded(key.blob, slices[r], d1, set_idx, bad, *RAND)
            except BaseException as e:      # noqa
                errs[r] = e
            finally:
                c.close()
        group = native.CommGroup(2)
        ts = [threading.Thread(target=body, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        group.close()
        assert not any(t.is_alive() for t in ts)
        assert all(isinstance(e, ValueError) and "does not satisfy" in str(e) for e in errs), errs
        assert str(errs[0]) == str(errs[1])                  # the same violated constraint (*bad) on every rank
    finally:
        key._slices = None
        for q in provers:
            q.close()


def test_groth16_over_ranks_a_failing_rank_frees_its_peers(wrap):
    """rank 1 passes a NULL slice of u1x it owns: ZP_ERR_ARG there, ZP_ERR_COMM on its peers -- an argument error, nothing reaches the GPU"""
    hip, wc, key, set_idx, set_val, _ = wrap
    G = 4
    provers = [native.Prover(0) for _ in range(G)]
    try:
        slices = key.load_slices(provers)
        d1 = G16._g1_words(B.mul(B.G, key.toxic["delta"]))
        errs = [None] * G

        def body(r):
            c = native.Comm(provers[r], r, G, group=group)
            try:
                c.set_timeout_ms(5000)
                dev = dict(slices[r])
                if r == 1:
                    assert dev["u1x"] is not None
                    dev["u1x"] = None
                c.groth16_prove_sharded(key.blob, dev, d1, set_idx, set_val, *RAND)
            except BaseException as e:      # noqa
                errs[r] = e
            finally:
                c.close()
        group = native.CommGroup(G)
        ts = [threading.Thread(target=body, args=(r,)) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        group.close()
        assert not any(t.is_alive() for t in ts), "a rank is stuck in a collective"
        assert all(isinstance(e, native.ZpError) for e in errs), errs
        assert errs[1].code == -1                                         # ZP_ERR_ARG
        assert all(e.code == -6 for r, e in enumerate(errs) if r != 1)     # ZP_ERR_COMM
    finally:
        key._slices = None
        for q in provers:
            q.close()


def test_groth16_sharded_on_rccl_with_a_world_of_one(wrap):
    """zp_groth16_prove_sharded on a real RCCL communicator of one rank (the whole key is its slice) = zp_groth16_prove"""
    hip, wc, key, set_idx, set_val, (p_ref, pub_ref, _) = wrap
    dev = key.load_points(hip)
    handles = {k: v[0] for k, v in dev.items() if k != "delta1"}
    handles["n_v"] = dev["v_wires"][1]
    d1 = G16._g1_words(dev["delta1"])
    a0, b0, c0, pub0, _ = hip.p.groth16_prove(key.blob, handles, d1, set_idx, set_val, *RAND)
    comm = native.Comm(hip.p, 0, 1, native.comm_unique_id())
    try:
        a, b, c, pub, ms = comm.groth16_prove_sharded(key.blob, handles, d1, set_idx, set_val, *RAND)
    finally:
        comm.close()
    assert (a == a0).all() and (b == b0).all() and (c == c0).all() and pub == pub0 == pub_ref
    assert {"pi_a": G16._g1_point(a), "pi_b": G16._g2_point(b), "pi_c": G16._g1_point(c)} == p_ref


def test_engine_final_proof_with_a_sharded_wrap_equals_the_one_rank_wrap(tmp_path):
    """EngineConfig(wrap_ranks=2): the same final request gives the same proof.json and public input as wrap_ranks=1 (deterministic blinding)"""
    from eigen_zeth_amd.service.engine import Engine, EngineConfig
    from eigen_zeth_amd.service.server import default_backend_factory
    addr = "479881985774944702531460751064278034642760119942"
    res = {}
    for ranks in (2, 1):
        eng = Engine(default_backend_factory(0), EngineConfig(air="chunk64", logn=14, chunks_per_block=1, groth16_seed="test", wrap_ranks=ranks))
        ch = eng.gen_batch_chunks("w", [3, 4], 12345, "evm")
        proofs = eng.gen_chunk_proofs("w", ch["task_id"], ch["chunk_count"], ch["batch_data"])
        agg = eng.aggregate("w", proofs[0]["proof"], proofs[1]["proof"])
        res[ranks] = eng.final("w", agg, "BN128", addr)
        st = eng.stage_timings["final/w"]
        assert all("groth16/msm/" + k in st for k in ("A", "B1", "B2", "l", "h"))
        assert st.get("groth16/ranks") == (2 if ranks == 2 else None)
        print("wrap_ranks=%d groth16 stages:" % ranks, json.dumps({k: round(v * 1e3, 2) if k != "groth16/ranks" else v for k, v in st.items() if k.startswith("groth16")}))
    assert res[2] == res[1]
