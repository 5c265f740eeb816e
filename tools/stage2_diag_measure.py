"""zp_stark_diagnose_stage2 measured on one GPU: chunk64 at 2^20 and 2^22 rows, trace resident, three traces -- the honest witness, the same with
one range value outside the table (one broken lookup), and a whole column of ONE value against one table row (the hot key: every row of the
lookup's column a and of the permutation's two columns lands in one slot).  Per trace: milliseconds per call with the wave's merge of equal keys
("s2_diag_merge") on and off, beside zp_stark_check_witness on the same trace, and the records checked against the host path's (ctx = NULL) once.
Medians of five after one warm-up.  Every size is a process of its own with its own time limit; the first that fails ends the run.  With
--parent-lib PATH the parent commit's library times zp_stark_check_witness on the same traces in processes of its own (it has no diagnosis).
Not a gate: the call runs after a refusal, not on the proving path.
python tools/stage2_diag_measure.py [--parent-lib PATH] [--logns 20,22] [--out profiles/stage2_diag.json]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from eigen_zeth_amd import native
from eigen_zeth_amd.stark import air as AIR

P = native.P


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def traces(air, prog, logn):
    """(name, trace) x 3; the stage-2 table of the blob says which columns the arguments read"""
    N = 1 << logn
    tab = 12 + int(prog[6]) + int(prog[7])
    (k1, pa, pb, _), (k2, la, lt, lm) = [[int(v) for v in prog[tab + 4 * j:tab + 4 * j + 4]] for j in range(2)]
    assert (k1, k2) == (1, 2) and pa == la
    honest, _ = native.synth_trace(air.trace_kind, logn, air.width, 11 + logn)
    yield "honest", honest
    broken = honest.copy()
    broken[la, 5] = int(honest[lt].max()) + 9          # the permutation's other column follows; the constraints that read the cell do not matter here
    broken[pb, int(np.nonzero(honest[pb] == honest[la, 5])[0][0])] = broken[la, 5]
    yield "one_broken_lookup", broken
    hot = honest.copy()
    hot[la] = 5
    hot[pb] = 5
    hot[lt] = np.arange(5, 5 + N, dtype=np.uint64)
    hot[lm] = 0
    hot[lm, 0] = N
    yield "one_value_column", hot


def child(role, logn):
    if role == "parent":
        native.SIGNATURES.pop("zp_stark_diagnose_stage2")
    air = AIR.get_air("chunk64")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    p = native.Prover(0)
    out = {"role": role, "logn": logn, "traces": {}}
    for name, tr in traces(air, prog, logn):
        pubs = [int(v) for v in native.synth_trace(air.trace_kind, logn, air.width, 11 + logn)[1]]
        d = p.upload(np.ascontiguousarray(tr))
        row = {"check_witness_ms": median_ms(lambda: p.check_witness(prog, d, pubs, logn))}
        if role != "parent":
            want = [r.words for r in native.diagnose_stage2_host(prog, tr, logn)]
            for merge in (1, 0):
                p.set_tuning("s2_diag_merge", merge)
                assert [r.words for r in p.diagnose_stage2(prog, d, logn)] == want, (name, merge)
                row["diagnose_ms_merge%d" % merge] = median_ms(lambda: p.diagnose_stage2(prog, d, logn))
            p.set_tuning("s2_diag_merge", 1)
            row["verdicts"] = [w[0] for w in want]
        d.free()
        out["traces"][name] = row
        print(json.dumps({name: row}), flush=True)
    p.close()
    print("S2DIAG " + json.dumps(out), flush=True)


def main():
    arg = lambda k, dflt: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else dflt
    out_path, parent = arg("--out", os.path.join("profiles", "stage2_diag.json")), arg("--parent-lib", None)
    res = {"air": "chunk64", "medians_of": 5, "sizes": {}}
    for logn in [int(v) for v in arg("--logns", "20,22").split(",")]:
        for role in ["new"] + (["parent"] if parent else []):
            env = dict(os.environ, **({"ZP_LIB_PATH": os.path.abspath(parent)} if role == "parent" else {}))
            run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", role, str(logn)], env=env,
                                 capture_output=True, text=True)
            sys.stdout.write(run.stdout)
            if run.returncode != 0:       # nothing more is started on the GPU after a step that failed
                sys.stderr.write(run.stderr)
                sys.exit("the %s library's step at 2^%d ended with status %d" % (role, logn, run.returncode))
            line = [l for l in run.stdout.splitlines() if l.startswith("S2DIAG ")][-1]
            res["sizes"].setdefault(str(logn), {})[role] = json.loads(line[7:])["traces"]
        if not parent:
            res["sizes"][str(logn)]["parent"] = "UNMEASURED"
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1], int(sys.argv[sys.argv.index("--child") + 2]))
    else:
        main()
