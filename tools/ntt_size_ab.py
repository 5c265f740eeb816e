"""Forward / inverse / extension-by-2 at 32 columns, 2^20 .. 2^26 rows, of ONE library (measurement tool; an A/B is a job that runs
this in fresh processes with and without ZP_LIB_PATH, alternating):
    python tools/ntt_size_ab.py <label> [lo hi] >> profiles/xyz.jsonl
One JSON line per size: three timed windows (host clock around 4-20 synchronised calls) of each transform, ms per call; at 2^24 also
the per-launch times of the forward transform (pass_timings)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from eigen_zeth_amd.native import Prover

label = sys.argv[1]
lo, hi = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (20, 26)
cols = 32
p = Prover(0)
block = np.random.default_rng(12).integers(0, 2**63, size=(cols, 1 << 20), dtype=np.uint64)   # below the modulus; the work does not depend on the values


def windows(call, calls):
    call()
    p.sync()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        p.sync()
        out.append(round((time.perf_counter() - t0) * 1e3 / calls, 4))
    return out


for logn in range(lo, hi + 1):
    x = np.tile(block, (1, 1 << (logn - 20)))
    d, o, e = p.upload(x), p.alloc(cols << logn), p.alloc(cols << (logn + 1))
    del x
    calls = max(4, min(20, 1 << (24 - logn + 2)))
    row = {"lib": label, "logn": logn, "cols": cols,
           "ntt_ms": windows(lambda: p.ntt(d, o, logn, cols), calls),
           "intt_ms": windows(lambda: p.intt(d, o, logn, cols), calls),
           "lde_ms": windows(lambda: p.lde(d, e, logn, 1, cols), calls)}
    if logn == 24:
        p.set_profiling(True)
        p.pass_timings()
        p.ntt(d, o, logn, cols)
        p.sync()
        row["forward_launches_ms"] = [[r, round(ms, 4)] for r, ms in p.pass_timings()]
        p.set_profiling(False)
    print(json.dumps(row), flush=True)
    for b in (d, o, e):
        b.free()
p.close()
