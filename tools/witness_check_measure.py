"""zp_stark_check_witness measured on one GPU: chunk64 at 2^20 and 2^22 rows, the trace resident in HBM, an honest witness (SATISFIED: no atomic
is issued), medians of five after one warm-up, in a fresh process.  (a) the check alone, wall clock per call and split by the stage clock
(zp_set_profiling) into the canonical pass / the stage-2 columns / the program kernel (with the sparse columns' periods and the upload of the
program); (b) zp_stark_prove of the same trace from the same library at the service's parameters, and the ratio check / proof -- what
EngineConfig(check_witness=True) adds to a chunk proof.  Recorded, not gated: the flag stays off by default whatever the number is.
python tools/witness_check_measure.py [--logn 20,22] [--out profiles/witness_check.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR

PARAMS = dict(logb=1, fri_logf=3, fri_final_log=5, n_queries=80, pow_bits=20)
STAGES = {"witness_canonical": "canonical_pass_ms", "witness_stage2": "stage2_columns_ms", "witness_program": "program_kernel_ms"}


def median(v):
    return round(sorted(v)[len(v) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", default="20,22")
    ap.add_argument("--out", default=os.path.join("profiles", "witness_check.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    p = native.Prover(0)
    air = AIR.get_air("chunk64")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    res = {"air": "chunk64", "width": air.width, "constraints": int(prog[8]), "instructions": int(prog[7]), "slots": int(prog[9]), "params": PARAMS,
           "device": p.device_info() if hasattr(p, "device_info") else None, "sizes": []}
    for logn in [int(v) for v in a.logn.split(",")]:
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 5)
        pubs = [int(v) for v in pub]
        d = p.upload(tr)
        del tr

        def check():
            rep = p.check_witness(prog, d, pubs, logn)
            assert rep.ok, str(rep)

        def prove():
            return p.stark_prove(air.name, prog, d, pubs, logn, PARAMS["logb"], PARAMS["fri_logf"], PARAMS["fri_final_log"], PARAMS["n_queries"], PARAMS["pow_bits"])
        check()
        wall, split = [], {k: [] for k in STAGES.values()}
        for _ in range(a.reps):
            p.set_profiling(True)
            p.stage_timings()
            t0 = time.perf_counter()
            check()
            wall.append((time.perf_counter() - t0) * 1e3)
            for ev in p.stage_timings():
                if ev["stage"] in STAGES:
                    split[STAGES[ev["stage"]]].append(ev["ms"])
            p.set_profiling(False)
        prove()
        tp = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            prove()
            tp.append((time.perf_counter() - t0) * 1e3)
        row = {"logn": logn, "trace_bytes": (air.width << logn) * 8, "check_ms": median(wall), "prove_ms": median(tp)}
        row.update({k: median(v) for k, v in split.items() if v})
        row["check_over_prove"] = round(row["check_ms"] / row["prove_ms"], 4)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        d.free()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    p.close()


if __name__ == "__main__":
    main()
