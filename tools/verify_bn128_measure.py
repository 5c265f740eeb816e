"""The BN128-hash-mode verifier, measured on one GPU at the shape of a final STARK over a verifier AIR: 47 columns, blow-up 4, fold by 8, final
2^5, 50 queries (the statement is the 47-column toy AIR: the verifier's work depends on the shape, not on the constraints).  (a) zp_stark_verify_bn128
of one text through a ctx on each job form ("verify16_lane_min": 17 lanes per hash job / one lane per job) and with ctx = NULL on 16 threads;
(b) zp_stark_verify_batch_bn128 over 1, 4 and 16 texts on each form, milliseconds per text; (c) the number of hash jobs of one text.
Medians of five runs after one warm-up; every verdict is checked to be ACCEPT.
python tools/verify_bn128_measure.py [out.json] [logn]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import prover as PR

COOP, LANE = 1 << 30, 1


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "verify_bn128.json")
    logn = int(sys.argv[2]) if len(sys.argv) > 2 else 14
    shape = (logn, 2, 3, 5, 50)
    p = native.Prover(0)
    p.install_poseidon_bn254(17)
    bn_tables = bn254_poseidon_params(17)
    air = AIR.wide_air(47)
    params = PR.StarkParams(*shape, hash="bn128")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    texts = []
    for seed in (5, 6, 7, 8):
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, seed)
        d = p.upload(tr)
        texts.append(p.stark_prove_bn128(air.name, prog, d, [int(v) for v in pub], *shape))
        d.free()
    q0 = json.loads(texts[0])["queries"][0]
    jobs = 50 * sum(1 + len(o["path"]) for o in [q0["trace"], q0["quotient"]] + q0["fri"])
    res = {"shape": dict(air="wide47", **params.to_dict()), "proof_bytes": len(texts[0]), "hash_jobs_per_text": jobs}

    def one(prover, threads=0):
        v = native.stark_verify_bn128(prog, texts[0], params, prover=prover, threads=threads, bn_tables=None if prover else bn_tables)
        assert v[0] == native.VERDICT_ACCEPT, v

    def batch(n):
        v = native.stark_verify_batch_bn128(prog, [texts[i % len(texts)] for i in range(n)], params, prover=p)
        assert v == [native.VERDICT_ACCEPT] * n, v

    res["one_text_ms"] = {"ctx_null_16_threads": median_ms(lambda: one(None, 16))}
    res["batch_ms_per_text"] = {}
    for form, knob in (("coop", COOP), ("lane", LANE)):
        p.set_tuning("verify16_lane_min", knob)
        res["one_text_ms"]["ctx_" + form] = median_ms(lambda: one(p))
        res["batch_ms_per_text"][form] = {str(n): round(median_ms(lambda: batch(n)) / n, 3) for n in (1, 4, 16)}
        print(json.dumps({form: [res["one_text_ms"]["ctx_" + form], res["batch_ms_per_text"][form]]}), flush=True)
    p.set_tuning("verify16_lane_min", 0)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    p.close()


if __name__ == "__main__":
    main()
