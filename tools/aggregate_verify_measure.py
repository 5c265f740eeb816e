"""The native verifier of aggregated proofs, measured on one GPU.
(a) zp_program_fixed_eval_ext_batch alone on the verifier AIR of the service's shape (the statement of an aggregation STARK over two
chunk64 proofs of 2^20 rows: ~10^2 sparse fixed columns, ~4 x 10^5 entries): the fixed columns at 1, 8 and 64 random points with random public
inputs, on the device ("fixed_eval_dev_min" = 0: tables already on the ctx, and the first call that makes them) and on the host (ctx = NULL, 16
threads and 1 thread), milliseconds per call and per point, and the smallest of the three counts at which the device is not slower -- what the default
of "fixed_eval_dev_min" (points x entries) should be set from.  Every device result is checked to be the host's, word for word.  Medians of five
runs after one warm-up.
(b) with `--texts`: zp_aggregate_verify of one level-1 text over two chunk64 proofs of 2^LOGN rows (default 20: the service's shape) and of the level-2
tree over four such proofs, through a ctx and with ctx = NULL on 16 threads, and header-only; every verdict is checked to be ACCEPT.
python tools/aggregate_verify_measure.py [out.json] [--texts [LOGN]]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.poseidon_constants import default_mds, default_round_constants
from eigen_zeth_amd.service.engine import EngineConfig, recursion_airs_for
from eigen_zeth_amd.stark import air as AIR
from eigen_zeth_amd.stark import verifier_air as VA

ROOT32, SHIFT = 1753635133440165772, 49


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def measure_texts(p, rc, mds, logn, res):
    """(b): a level-1 text and a level-2 tree at the service's parameters, made on the device"""
    import copy
    from eigen_zeth_amd.stark import prover as PR
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    hip = HipBackend(prover=p)
    cfg = EngineConfig(air="chunk64", logn=logn)
    air = AIR.get_air(cfg.air)
    params = PR.StarkParams(logn, cfg.logb, cfg.fri_logf, cfg.fri_final_log, cfg.n_queries, pow_bits=cfg.pow_bits)
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    strip = lambda pr: {k: copy.deepcopy(v) for k, v in pr.items() if k != "queries"}

    def aggregate(proofs, digest_words, n_queries):
        shape = VA.Shape.of_proof(proofs[0], len(proofs))
        vair = VA.verifier_air(shape, rc, mds)
        d_trace, pubs = VA.build_witness(shape, proofs, hip, digest_words)
        ap = VA.aggregation_params(shape, n_queries, cfg.fri_logf, cfg.fri_final_log, cfg.agg_pow_bits)
        stark = json.loads(hip.prove_native(vair, d_trace, pubs, ap))
        return shape, vair, ap, {"shape": shape.to_dict(), "inner": [strip(pr) for pr in proofs], "stark": stark}
    chunk = []
    for seed in (5, 6, 7, 8):
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, seed)
        d = p.upload(tr)
        chunk.append(json.loads(p.stark_prove(air.name, prog, d, [int(v) for v in pub], logn, cfg.logb, cfg.fri_logf, cfg.fri_final_log, cfg.n_queries, cfg.pow_bits)))
        d.free()
    shape1, vair1, ap1, A = aggregate(chunk[:2], air.digest_words(), cfg.agg_queries)
    B = aggregate(chunk[2:], air.digest_words(), cfg.agg_queries)[3]
    shape2, vair2, ap2, top = aggregate([A["stark"], B["stark"]], vair1.digest_words(), cfg.agg_queries)
    top["children"] = [{"shape": A["shape"], "inner": A["inner"]}, {"shape": B["shape"], "inner": B["inner"]}]
    statements = [(None, prog, params, 0), (shape1.to_dict(), vair1.program(), ap1, shape1.n_slots()), (shape2.to_dict(), vair2.program(), ap2, shape2.n_slots())]
    out = {"chunk_logn": logn, "headers": {"level1": 2, "level2": 6}}
    for name, obj in (("level1", A), ("level2", top)):
        text = json.dumps(obj)

        def run(prover, flags=0, threads=16):
            v = native.aggregate_verify(statements, text, flags, prover=prover, threads=threads)
            assert v == (native.VERDICT_ACCEPT, -1), v
        out[name] = {"text_bytes": len(text), "ctx_ms": median_ms(lambda: run(p)), "ctx_null_16_threads_ms": median_ms(lambda: run(None)),
                     "ctx_header_only_ms": median_ms(lambda: run(p, native.VERIFY_HEADER_ONLY)),
                     "ctx_null_header_only_ms": median_ms(lambda: run(None, native.VERIFY_HEADER_ONLY))}
        print(json.dumps({name: out[name]}), flush=True)
    res["texts"] = out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join("profiles", "r12_fixed_eval_batch.json")
    rc, mds = np.array(default_round_constants(), dtype=np.uint64), np.array(default_mds(), dtype=np.uint64)
    cfg = EngineConfig(air="chunk64", logn=20)
    vair, _ = recursion_airs_for(cfg, ROOT32, SHIFT, rc, mds)
    prog = np.ascontiguousarray(vair.program(), dtype=np.uint64)
    air = AIR.get_air(cfg.air)
    chunk_shape = VA.Shape(cfg.logn, cfg.logb, air.width, air.width2, 3 * AIR.quotient_chunks(air), cfg.n_queries, cfg.fri_logf, cfg.fri_final_log, 2, air.n_pub,
                           cfg.pow_bits, ROOT32, SHIFT)
    logn = VA.aggregation_params(chunk_shape, cfg.agg_queries, cfg.fri_logf, cfg.fri_final_log, cfg.agg_pow_bits).logn      # rows of the aggregation STARK's trace
    n_pub = int(prog[4])
    entries = 0
    at = 12 + int(prog[6]) + int(prog[7]) + 4 * int(prog[10])
    lps = []
    for _ in range(int(prog[3]) - 2):
        lps.append(int(prog[at]) & 0xFF)
        entries += int(prog[at]) >> 8
        at += 1 + 2 * (int(prog[at]) >> 8)
    assert max(lps) <= logn
    res = {"program_words": int(prog.size), "sparse_columns": len(lps), "entries": entries, "n_pub": n_pub, "logn": logn}
    print(json.dumps(res), flush=True)
    p = native.Prover(0)
    rng = np.random.default_rng(12)
    res["by_points"], cross = {}, None
    for n in (1, 8, 64):
        zeta = rng.integers(0, native.P, size=(n, 3), dtype=np.uint64)
        pubs = rng.integers(0, native.P, size=(n, n_pub), dtype=np.uint64)
        host, hflags = native.program_fixed_eval_ext_batch(prog, pubs, logn, ROOT32, zeta, threads=16)
        p.set_tuning("fixed_eval_dev_min", 0)
        dev, dflags = native.program_fixed_eval_ext_batch(prog, pubs, logn, ROOT32, zeta, prover=p)
        assert (dev == host).all() and (dflags == hflags).all() and not hflags.any()
        row = {"device_ms": median_ms(lambda: native.program_fixed_eval_ext_batch(prog, pubs, logn, ROOT32, zeta, prover=p)),
               "host_16_threads_ms": median_ms(lambda: native.program_fixed_eval_ext_batch(prog, pubs, logn, ROOT32, zeta, threads=16)),
               "host_1_thread_ms": median_ms(lambda: native.program_fixed_eval_ext_batch(prog, pubs, logn, ROOT32, zeta, threads=1), reps=3)}
        row["device_ms_per_point"] = round(row["device_ms"] / n, 3)
        row["host_16_threads_ms_per_point"] = round(row["host_16_threads_ms"] / n, 3)
        res["by_points"][str(n)] = row
        if cross is None and row["device_ms"] <= row["host_16_threads_ms"]:
            cross = n
        print(json.dumps({n: row}), flush=True)
    p.set_tuning("fixed_eval_dev_min", -1)
    res["device_not_slower_from_points"] = cross
    # the first call on a fresh ctx: the per-entry tables are made on the host and uploaded
    q = native.Prover(0)
    q.set_tuning("fixed_eval_dev_min", 0)
    t0 = time.perf_counter()
    native.program_fixed_eval_ext_batch(prog, pubs[:1], logn, ROOT32, zeta[:1], prover=q)
    res["first_call_with_table_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    q.close()
    if "--texts" in sys.argv:
        measure_texts(p, rc, mds, int(args[1]) if len(args) > 1 else 20, res)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    p.close()


if __name__ == "__main__":
    main()
