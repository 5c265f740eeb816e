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
    own run-to-run spread, or the refactoring has cost something.

--sharded (profiles/witness_check_sharded.json): what "prove_check" adds to zp_stark_prove_sharded, chunk64 at --logn (default 20): a world of one on
RCCL and four thread-ranks on the one GPU (an in-process communicator: the ranks share the GPU's CUs -- a REHEARSAL of the multi-rank path, not a
multi-GPU number).  One child process per shape; in it knob 0 and knob 1 ALTERNATE, --reps proofs each after a warm-up of both; wall clock of the slowest
rank per proof, and under knob 1 rank 0's stage clock: canonical pass, exchange, row-window program kernel, each separately."""
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
          "witness_program_gen": "program_kernel_ms", "witness_exchange": "exchange_ms", "witness_program_rows": "program_kernel_ms",
          "witness_program_rows_gen": "program_kernel_ms"}


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


def sharded_child(a):
    """one shape in this process: --ranks 1 = a world of one on RCCL, else thread-ranks on GPU 0.  Prints ONE JSON line"""
    import threading
    logn, G = int(a.logn), a.ranks
    air = AIR.get_air("chunk64")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 5)
    pubs = [int(v) for v in pub]
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    group = native.CommGroup(G) if G > 1 else None
    uid = native.comm_unique_id() if G == 1 else None
    gate = threading.Barrier(G)
    wall = {0: [[] for _ in range(G)], 1: [[] for _ in range(G)]}
    split, errs, texts = {}, [], set()

    def rank(r):
        try:
            p = native.Prover(0)
            be = HipBackend(prover=p)
            c = native.Comm(p, r, G, unique_id=uid, group=group)
            p.set_air_kernel_rows(prog, be._airlib_rows(air))
            p.set_air_kernel_witness_rows(prog, be._airlib_witness_rows(air))
            p.set_tuning("witness_kernel", a.witness_kernel)
            first, count = c.my_columns(air.width)
            d = p.upload(np.ascontiguousarray(tr[first:first + count]))

            def prove(knob, timed):
                p.set_tuning("prove_check", knob)
                p.set_profiling(timed and r == 0)
                p.stage_timings()
                p.sync()
                gate.wait()
                t0 = time.perf_counter()
                texts.add(c.stark_prove_sharded(air.name, prog, d, pubs, logn, PARAMS["logb"], PARAMS["fri_logf"], PARAMS["fri_final_log"], PARAMS["n_queries"],
                                                PARAMS["pow_bits"]))
                if timed:
                    wall[knob][r].append((time.perf_counter() - t0) * 1e3)
                    if r == 0 and knob:
                        for ev in p.stage_timings():
                            if ev["stage"] in STAGES:
                                split.setdefault(STAGES[ev["stage"]], []).append(ev["ms"])
                                split.setdefault("stages_seen", set()).add(ev["stage"])
                p.set_profiling(False)
            for knob in (0, 1):
                prove(knob, False)
            for _ in range(a.reps):
                for knob in (0, 1):                         # alternating: both see the same neighbours on the machine
                    prove(knob, True)
            d.free()
            c.close()
            p.close()
        except BaseException as e:      # noqa: the other ranks must not wait for this one
            errs.append(e)
            gate.abort()
    ts = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    assert len(texts) == 1, "knob 0 and knob 1 must give the same bytes on every rank"
    seen = sorted(split.pop("stages_seen", []))
    row = {"logn": logn, "ranks": G, "transport": "rccl" if G == 1 else "threads on one GPU (rehearsal)", "witness_kernel": a.witness_kernel, "reps": a.reps}
    for knob in (0, 1):
        per_proof = [max(wall[knob][r][i] for r in range(G)) for i in range(a.reps)]          # a proof is done when its slowest rank is
        row["prove_check_%d" % knob] = {"ms": median(per_proof), "ms_min": round(min(per_proof), 4), "ms_max": round(max(per_proof), 4)}
    row["check_over_proof"] = round(row["prove_check_1"]["ms"] / row["prove_check_0"]["ms"] - 1, 4)
    row["stages"] = seen
    row.update({k: median(v) for k, v in split.items()})
    print(json.dumps(row), flush=True)


def sharded(a):
    import subprocess
    here = os.path.abspath(__file__)
    air = AIR.get_air("chunk64")
    res = {"air": "chunk64", "width": air.width, "constraints": len(air.constraints), "params": PARAMS,
           "note": "thread-ranks share one GPU: a rehearsal of the multi-rank path, not a multi-GPU number", "shapes": []}
    for logn in [int(v) for v in a.logn.split(",")]:
        for G in (1, 4):
            cmd = [sys.executable, here, "--sharded-child", "--logn", str(logn), "--ranks", str(G), "--reps", str(a.reps), "--witness-kernel", str(a.witness_kernel)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)          # a time limit per GPU step; TimeoutExpired ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("step %s failed with status %d: nothing more is started" % (cmd[2:], r.returncode))
            row = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            res["shapes"].append(row)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


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
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--sharded-child", action="store_true")
    ap.add_argument("--ranks", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.sharded_child:
        return sharded_child(a)
    if a.sharded:
        a.out = a.out or os.path.join("profiles", "witness_check_sharded.json")
        if a.logn == "20,22":
            a.logn = "20"
        return sharded(a)
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
