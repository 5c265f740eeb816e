"""The Groth16 wrap over the ranks (zp_groth16_prove_sharded), measured on one GPU at the service's size (the wrap of a final STARK over two
chunk proofs of 2^14 rows: a 2^22 QAP domain, 2.8-4.2 M points per MSM): (1) h_ms on an RCCL communicator of one rank against zp_groth16_prove
on the same key -- five alternating runs each after one warm-up, medians; (2) the wall time of the wrap over 8 thread-ranks sharing the GPU (a
rehearsal of the path: the ranks share one GPU's CUs, no speed-up is expected).  Every proof.json is checked against the first one.
python tools/wrap_sharded_measure.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.service import groth16 as G16
from eigen_zeth_amd.service.engine import Engine, EngineConfig
from eigen_zeth_amd.service.server import default_backend_factory

addr = "479881985774944702531460751064278034642760119942"
eng = Engine(default_backend_factory(0), EngineConfig(air="chunk64", logn=14, chunks_per_block=1, groth16_seed="m"))
ch = eng.gen_batch_chunks("w", [3, 4], 12345, "evm")
proofs = eng.gen_chunk_proofs("w", ch["task_id"], ch["chunk_count"], ch["batch_data"])
agg = eng.aggregate("w", proofs[0]["proof"], proofs[1]["proof"])
base = eng.final("w", agg, "BN128", addr)
comm = native.Comm(eng.be.p, 0, 1, native.comm_unique_id())
orig = G16.prove


def prove_rccl(key, set_idx, set_val, be, rand):
    dev = key.load_points(be)
    h = {k: v[0] for k, v in dev.items() if k != "delta1"}
    h["n_v"] = dev["v_wires"][1]
    a, b, c, pub, ms = comm.groth16_prove_sharded(key.blob, h, G16._g1_words(dev["delta1"]), set_idx, set_val, *rand)
    return {"pi_a": G16._g1_point(a), "pi_b": G16._g2_point(b), "pi_c": G16._g1_point(c)}, pub, ms


rows = {"one_ctx": [], "rccl_world1": []}
for it in range(6):
    for mode in ("one_ctx", "rccl_world1"):
        G16.prove = orig if mode == "one_ctx" else prove_rccl
        out = eng.final("w", agg, "BN128", addr)
        assert out == base, mode
        st = eng.stage_timings["final/w"]
        rows[mode].append({k: st[k] * 1e3 for k in ("groth16", "groth16/witness", "groth16/qap", "groth16/msm")})
G16.prove = orig
comm.close()
med = lambda xs: sorted(xs)[len(xs) // 2]
summ = {m: {k: round(med([r[k] for r in v[1:]]), 2) for k in v[0]} for m, v in rows.items()}
hms = {m: round(summ[m]["groth16/witness"] + summ[m]["groth16/qap"] + summ[m]["groth16/msm"], 2) for m in summ}
print(json.dumps({"median_ms_of_5_after_warmup": summ, "h_ms_total": hms, "ratio": round(hms["rccl_world1"] / hms["one_ctx"], 4)}), flush=True)
res = {"wrap_info": eng.wrap_info, "rccl_world1_vs_one_ctx": {"median_ms_of_5_after_warmup": summ, "h_ms_total": hms,
       "ratio_rccl_over_one_ctx": round(hms["rccl_world1"] / hms["one_ctx"], 4)}}
walls = []
for ranks in (8,):
    eng.cfg.wrap_ranks = ranks
    t0 = time.perf_counter()
    out = eng.final("w", agg, "BN128", addr)
    t_first = time.perf_counter() - t0           # includes making the 8 key slices
    assert out == base
    for it in range(3):
        out = eng.final("w", agg, "BN128", addr)
        assert out == base
        st = eng.stage_timings["final/w"]
        walls.append({k: round(v * 1e3, 2) if k != "groth16/ranks" else v for k, v in st.items() if k.startswith("groth16")})
    res["thread_ranks_8_one_gpu"] = {"first_call_with_key_slices_s": round(t_first, 3), "runs_ms": walls}
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
