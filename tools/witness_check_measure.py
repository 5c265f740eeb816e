"""zp_stark_check_witness measured on one GPU: chunk64 at 2^20 and 2^22 rows, the trace resident in HBM, an honest witness (SATISFIED: no atomic
is issued), medians of five after one warm-up, in a fresh process.  (a) the check alone, wall clock per call and split by the stage clock
(zp_set_profiling) into the canonical pass / the stage-2 columns / the program kernel (with the sparse columns' periods and the upload of the
program); (b) zp_stark_prove of the same trace from the same library at the service's parameters, and the ratio check / proof -- what
EngineConfig(check_witness=True) adds to a chunk proof.  Recorded, not gated: the flag stays off by default whatever the number is.
python tools/witness_check_measure.py [--logn 20,22] [--out profiles/witness_check.json]

--inproof (profiles/witness_check_inproof.json): the check INSIDE the proof and the generated witness kernel, same sizes, same rules.  Every GPU step
is a child process of its own with its own time limit (a step that fails or runs out of time ends the whole measurement: nothing more is started):
(a) the stand-alone check with the interpreter ("witness_kernel" 0) and with the generated kernel (1), split by the stage clock;
(b) zp_stark_prove with "prove_check" 0 and 1, for each kernel form, wall clock, and under 1 the stage clock's canonical pass and program kernel;
(c) "prove_check" 0 of this library against ANOTHER build of the library (--parent-lib: the parent commit's), as child processes of the two libraries
    alternating, --rounds each; per library the median of its processes' medians and their spread (max - min).  The new library sits inside the parent's
    own run-to-run spread, or the refactoring has cost something."""
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
STAGES = {"witness_canonical": "canonical_pass_ms", "witness_stage2": "stage2_columns_ms", "witness_program": "program_kernel_ms",
          "witness_program_gen": "program_kernel_ms"}


def median(v):
    return round(sorted(v)[len(v) // 2], 4)


def spread(v):
    return round(max(v) - min(v), 4)


def child(a):
    """one GPU step in this process: prints ONE JSON line.  --step check | prove; --witness-kernel 0 | 1; --prove-check 0 | 1"""
    logn = int(a.logn)
    old = a.no_new_calls                                   # another build of the library (the parent commit's): no knob, no witness kernel, and the
    if old:                                                # binding table must not ask it for the calls it does not export
        for name in ("zp_stark_set_air_kernel_witness", "zp_stark_prove_witness_report"):
            native.SIGNATURES.pop(name, None)
    p = native.Prover(0)
    air = AIR.get_air("chunk64")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 5)
    pubs = [int(v) for v in pub]
    d = p.upload(tr)
    del tr
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    be = HipBackend(prover=p)                              # the same set-up for both libraries: only the new calls differ
    p.set_air_kernel(prog, be._airlib(air))
    if not old:
        p.set_air_kernel_witness(prog, be._airlib_witness(air))
        p.set_tuning("witness_kernel", a.witness_kernel)
        p.set_tuning("prove_check", a.prove_check)

    def check():
        rep = p.check_witness(prog, d, pubs, logn)
        assert rep.ok, str(rep)

    def prove():
        return p.stark_prove(air.name, prog, d, pubs, logn, PARAMS["logb"], PARAMS["fri_logf"], PARAMS["fri_final_log"], PARAMS["n_queries"], PARAMS["pow_bits"])
    call = check if a.step == "check" else prove
    call()
    wall, split = [], {}
    for _ in range(a.reps):
        p.set_profiling(True)
        p.stage_timings()
        p.sync()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for ev in p.stage_timings():
            if ev["stage"] in STAGES:
                split.setdefault(STAGES[ev["stage"]], []).append(ev["ms"])
                split.setdefault("stages_seen", set()).add(ev["stage"])
        p.set_profiling(False)
    seen = sorted(split.pop("stages_seen", []))
    row = {"step": a.step, "logn": logn, "witness_kernel": a.witness_kernel, "prove_check": a.prove_check, "ms": median(wall), "ms_min": round(min(wall), 4),
           "ms_max": round(max(wall), 4), "stages": seen}
    row.update({k: median(v) for k, v in split.items()})
    print(json.dumps(row), flush=True)
    d.free()
    p.close()


def inproof(a):
    import subprocess
    here = os.path.abspath(__file__)
    parent_lib = os.path.abspath(a.parent_lib) if a.parent_lib else None

    def step(logn, what, wk=1, pc=0, lib=None, limit=240):
        env = dict(os.environ)
        if lib:
            env["ZP_LIB_PATH"] = lib
        cmd = [sys.executable, here, "--child", "--logn", str(logn), "--step", what, "--witness-kernel", str(wk), "--prove-check", str(pc), "--reps", str(a.reps)]
        if lib:
            cmd.append("--no-new-calls")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)          # a time limit per GPU step; TimeoutExpired ends the run
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("step %s failed with status %d: nothing more is started" % (cmd[3:], r.returncode))
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        return row
    air = AIR.get_air("chunk64")
    res = {"air": "chunk64", "width": air.width, "constraints": len(air.constraints), "params": PARAMS, "reps_per_process": a.reps, "sizes": []}
    for logn in [int(v) for v in a.logn.split(",")]:
        out = {"logn": logn, "trace_bytes": (air.width << logn) * 8}
        out["a_check_alone"] = {"interpreter": step(logn, "check", wk=0), "generated": step(logn, "check", wk=1)}
        out["b_prove"] = {"prove_check_0": step(logn, "prove", wk=1, pc=0), "prove_check_1_interpreter": step(logn, "prove", wk=0, pc=1),
                          "prove_check_1_generated": step(logn, "prove", wk=1, pc=1)}
        base = out["b_prove"]["prove_check_0"]["ms"]
        for k in ("prove_check_1_interpreter", "prove_check_1_generated"):
            out["b_prove"][k + "_over_0"] = round(out["b_prove"][k]["ms"] / base - 1, 4)
        if parent_lib:
            new, old = [], []
            for _ in range(a.rounds):
                old.append(step(logn, "prove", lib=parent_lib)["ms"])
                new.append(step(logn, "prove", wk=1, pc=0)["ms"])
            out["c_prove_check_0_against_parent"] = {"parent_ms": old, "this_ms": new, "parent_median": median(old), "this_median": median(new),
                                                     "parent_spread": spread(old), "this_spread": spread(new),
                                                     "inside_parent_spread": bool(min(old) <= median(new) <= max(old))}
        res["sizes"].append(out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", default="20,22")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inproof", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--step", default="check")
    ap.add_argument("--witness-kernel", type=int, default=1)
    ap.add_argument("--prove-check", type=int, default=0)
    ap.add_argument("--no-new-calls", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.inproof:
        a.out = a.out or os.path.join("profiles", "witness_check_inproof.json")
        return inproof(a)
    a.out = a.out or os.path.join("profiles", "witness_check.json")
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
