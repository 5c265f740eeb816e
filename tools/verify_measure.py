"""The native STARK verifier, measured on one GPU at the service's shape (chunk64, 2^20 rows, blow-up 2, fold by 8, final 2^5, 80 queries, 20
grinding bits): (a) zp_stark_verify of one proof through a ctx and with ctx = NULL, and with ZP_VERIFY_HEADER_ONLY on one thread -- everything
but the queries, all host code: text header, Fiat-Shamir transcript on the host Poseidon, identity at zeta, final-layer degree; an UPPER bound on
what the host transcript costs per proof; (b) zp_stark_verify_batch over 1, 4, 16 and 64 proofs,
milliseconds per proof, openings on the lane-per-opening kernel and on the 12-lane walk kernel ("verify_lane_min"); (c) zp_merkle_verify_batch
alone (leaves of 24 values, depth 16: a FRI layer's openings) at 16 .. 8192 openings on both kernels, and the count from which the lane kernel is
the faster one -- the default of "verify_lane_min".  Medians of five runs after one warm-up; every verdict is checked to be ACCEPT.
python tools/verify_measure.py [out.json]
--chains: the transcripts as device sponge chains ("verify_chain_dev") for batches of 1 / 4 / 16 / 64 chunk proofs with the knob at 0 and at 2, the
counters of zp_verify_counters, and with --parent-lib PATH the parent commit's library alternating with the new one (tools/verify_bn128_measure.py
has the driver).  Merged into profiles/verify_chains.json under "goldilocks".
python tools/verify_measure.py --chains [--parent-lib PATH] [--rounds 3] [--logn 20] [--out profiles/verify_chains.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR

LANE, WALK = 1, 1 << 30
SHAPE = (20, 1, 3, 5, 80, 20)


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r9_verify.json")
    p = native.Prover(0)
    air = AIR.get_air("chunk64")
    params = PR.StarkParams(*SHAPE[:5], pow_bits=SHAPE[5])
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    texts = []
    for seed in (5, 6, 7, 8):
        tr, pub = native.synth_trace(air.trace_kind, SHAPE[0], air.width, seed)
        d = p.upload(tr)
        texts.append(p.stark_prove(air.name, prog, d, [int(v) for v in pub], *SHAPE))
        d.free()
    res = {"shape": dict(air="chunk64", **params.to_dict()), "proof_bytes": len(texts[0])}

    def one(prover):
        v = native.stark_verify(prog, texts[0], params, prover=prover)
        assert v[0] == native.VERDICT_ACCEPT, v

    def header_only():
        v = native.stark_verify(prog, texts[0], params, native.VERIFY_HEADER_ONLY, threads=1)
        assert v[0] == native.VERDICT_ACCEPT, v

    res["one_proof_ms"] = {"ctx": median_ms(lambda: one(p)), "ctx_null": median_ms(lambda: one(None)), "header_only_host_one_thread": median_ms(header_only)}
    print(json.dumps(res), flush=True)

    def batch(n):
        v = native.stark_verify_batch(prog, [texts[i % len(texts)] for i in range(n)], params, prover=p)
        assert v == [native.VERDICT_ACCEPT] * n, v

    res["batch_ms_per_proof"] = {}
    for form, knob in (("lane", LANE), ("walk", WALK)):
        p.set_tuning("verify_lane_min", knob)
        res["batch_ms_per_proof"][form] = {str(n): round(median_ms(lambda: batch(n)) / n, 3) for n in (1, 4, 16, 64)}
        print(json.dumps({form: res["batch_ms_per_proof"][form]}), flush=True)

    # (c) the opening kernels alone
    width, depth = 24, 16
    M = 1 << depth
    rng = np.random.default_rng(9)
    cols = rng.integers(0, native.P, size=(width, M), dtype=np.uint64)
    d_cols, d_tree = p.upload(cols), p.alloc((2 * M - 1) * 4)
    p.merkle_commit(d_cols, M, width, d_tree)
    tree = p.download(d_tree, (2 * M - 1, 4))
    sweep, cross = {}, None
    for n in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
        index = rng.integers(0, M, size=n, dtype=np.uint64)
        values = np.ascontiguousarray(cols[:, index.astype(np.int64)].T)
        paths = np.zeros((n, depth, 4), dtype=np.uint64)
        for o in range(n):
            pos, off, cnt = int(index[o]), 0, M
            for lv in range(depth):
                paths[o, lv] = tree[off + (pos ^ 1)]
                off, cnt, pos = off + cnt, cnt >> 1, pos >> 1
        row = {}
        for form, knob in (("lane", LANE), ("walk", WALK)):
            p.set_tuning("verify_lane_min", knob)

            def run():
                assert p.merkle_verify_batch(values, index, paths, tree[-1]).all()
            row[form] = median_ms(run)
        sweep[str(n)] = row
        if cross is None and row["lane"] <= row["walk"]:
            cross = n
        print(json.dumps({n: row}), flush=True)
    p.set_tuning("verify_lane_min", 0)
    res["openings_ms"] = {"width": width, "depth": depth, "by_count": sweep, "lane_not_slower_from": cross}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    p.close()


def chains_child(role, logn):
    """one library, one process: ms per call of every batch size (a parent library has neither the knob nor the counters)"""
    if role == "parent":
        for name in ("zp_poseidon_bn254_chains", "zp_verify_counters"):
            native.SIGNATURES.pop(name)
    shape = (logn,) + SHAPE[1:]
    p = native.Prover(0)
    air = AIR.get_air("chunk64")
    params = PR.StarkParams(*shape[:5], pow_bits=shape[5])
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    texts = []
    for seed in (5, 6, 7, 8):
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, seed)
        d = p.upload(tr)
        texts.append(p.stark_prove(air.name, prog, d, [int(v) for v in pub], *shape))
        d.free()

    def batch(n):
        v = native.stark_verify_batch(prog, [texts[i % len(texts)] for i in range(n)], params, prover=p)
        assert v == [native.VERDICT_ACCEPT] * n, v

    out = {"role": role, "ms_per_call": {}}
    for knob in ((None,) if role == "parent" else (0, 2)):
        if knob is not None:
            p.set_tuning("verify_chain_dev", knob)
        before = native.verify_counters(p) if knob is not None else None
        row = {str(n): median_ms(lambda: batch(n)) for n in (1, 4, 16, 64)}
        if knob is not None:
            after = native.verify_counters(p)
            row["counters"] = {k: after[k] - before[k] for k in after}
        out["ms_per_call"]["parent" if knob is None else "knob%d" % knob] = row
    p.close()
    print("CHAINS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    if "--chains-child" in sys.argv:
        chains_child(sys.argv[sys.argv.index("--chains-child") + 1], int(sys.argv[sys.argv.index("--chains-child") + 2]))
    elif "--chains" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from verify_bn128_measure import chains_main
        chains_main(sys.argv, "goldilocks", [sys.argv[sys.argv.index("--logn") + 1] if "--logn" in sys.argv else str(SHAPE[0])], script=__file__)
    else:
        main()
