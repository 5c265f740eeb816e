"""The BN128-hash-mode verifier, measured on one GPU at the shape of a final STARK over a verifier AIR: 47 columns, blow-up 4, fold by 8, final
2^5, 50 queries (the statement is the 47-column toy AIR: the verifier's work depends on the shape, not on the constraints).  (a) zp_stark_verify_bn128
of one text through a ctx on each job form ("verify16_lane_min": 17 lanes per hash job / one lane per job) and with ctx = NULL on 16 threads;
(b) zp_stark_verify_batch_bn128 over 1, 4 and 16 texts on each form, milliseconds per text; (c) the number of hash jobs of one text.
Medians of five runs after one warm-up; every verdict is checked to be ACCEPT.
python tools/verify_bn128_measure.py [out.json] [logn]
--chains: the transcripts as device sponge chains ("verify_chain_dev").  Batches of 1 / 4 / 16 texts with the knob at 0 and at 2, medians of five, and
the counters of zp_verify_counters; with --parent-lib PATH (a libzethprover.so built from the parent commit) the same batches through that library,
in child processes that alternate with the new library's -- the speed yardstick is the parent, not knob 0.  Merged into profiles/verify_chains.json
under "bn128".
python tools/verify_bn128_measure.py --chains [--parent-lib PATH] [--rounds 3] [--logn 14] [--out profiles/verify_chains.json]"""
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


def chains_child(role, logn):
    """one library, one process: ms per call of every batch size (a parent library has neither the knob nor the counters)"""
    if role == "parent":
        for name in ("zp_poseidon_bn254_chains", "zp_verify_counters"):
            native.SIGNATURES.pop(name)
    shape = (logn, 2, 3, 5, 50)
    p = native.Prover(0)
    p.install_poseidon_bn254(17)
    air = AIR.wide_air(47)
    params = PR.StarkParams(*shape, hash="bn128")
    prog = np.ascontiguousarray(air.program(), dtype=np.uint64)
    texts = []
    for seed in (5, 6, 7, 8):
        tr, pub = native.synth_trace(air.trace_kind, logn, air.width, seed)
        d = p.upload(tr)
        texts.append(p.stark_prove_bn128(air.name, prog, d, [int(v) for v in pub], *shape))
        d.free()

    def batch(n):
        v = native.stark_verify_batch_bn128(prog, [texts[i % len(texts)] for i in range(n)], params, prover=p)
        assert v == [native.VERDICT_ACCEPT] * n, v

    out = {"role": role, "ms_per_call": {}}
    for knob in ((None,) if role == "parent" else (0, 2)):
        if knob is not None:
            p.set_tuning("verify_chain_dev", knob)
        before = native.verify_counters(p) if knob is not None else None
        row = {str(n): median_ms(lambda: batch(n)) for n in (1, 4, 16)}
        if knob is not None:
            after = native.verify_counters(p)
            row["counters"] = {k: after[k] - before[k] for k in after}
        out["ms_per_call"]["parent" if knob is None else "knob%d" % knob] = row
    p.close()
    print("CHAINS " + json.dumps(out), flush=True)


def chains_main(argv, mode, child_args, script=None):
    """alternates child processes of the parent library and of the new one; this process never opens the GPU"""
    import subprocess

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default
    parent_lib, rounds, out_path = opt("--parent-lib", None), int(opt("--rounds", "3")), opt("--out", os.path.join("profiles", "verify_chains.json"))
    runs = {"parent": [], "new": []}
    for _ in range(rounds):
        for role in (("parent", "new") if parent_lib else ("new",)):
            env = dict(os.environ)
            if role == "parent":
                env["ZP_LIB_PATH"] = os.path.abspath(parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(script or __file__), "--chains-child", role] + child_args, env=env, capture_output=True, text=True, timeout=1500)
            line = [l for l in r.stdout.splitlines() if l.startswith("CHAINS ")]
            if r.returncode != 0 or not line:
                raise SystemExit("child %s failed:\n%s\n%s" % (role, r.stdout[-2000:], r.stderr[-2000:]))
            runs[role].append(json.loads(line[0][7:])["ms_per_call"])
            print(role, json.dumps(runs[role][-1]), flush=True)
    sizes = [k for k in runs["new"][0]["knob2"] if k != "counters"]
    res = {"rounds": rounds, "sizes": sizes, "new_knob0_ms": {n: [r["knob0"][n] for r in runs["new"]] for n in sizes},
           "new_knob2_ms": {n: [r["knob2"][n] for r in runs["new"]] for n in sizes}, "counters_knob2": runs["new"][-1]["knob2"]["counters"],
           "counters_knob0": runs["new"][-1]["knob0"]["counters"]}
    if parent_lib:
        res["parent_ms"] = {n: [r["parent"][n] for r in runs["parent"]] for n in sizes}
        # default-on stays only where the new library (knob 2) beats the parent at every size by more than the parent's own run-to-run spread
        verdict = {}
        for n in sizes:
            par, new = sorted(res["parent_ms"][n]), sorted(res["new_knob2_ms"][n])
            verdict[n] = {"parent_median": par[len(par) // 2], "parent_spread": round(par[-1] - par[0], 3), "new_median": new[len(new) // 2]}
            verdict[n]["faster_by_more_than_spread"] = verdict[n]["parent_median"] - verdict[n]["new_median"] > verdict[n]["parent_spread"]
        res["against_parent"] = verdict
        res["device_wins_at_every_size"] = all(v["faster_by_more_than_spread"] for v in verdict.values())
    else:
        res["parent_ms"] = "UNMEASURED"
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc[mode] = res
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if "--chains-child" in sys.argv:
        chains_child(sys.argv[sys.argv.index("--chains-child") + 1], int(sys.argv[sys.argv.index("--chains-child") + 2]))
    elif "--chains" in sys.argv:
        chains_main(sys.argv, "bn128", [sys.argv[sys.argv.index("--logn") + 1] if "--logn" in sys.argv else "14"])
    else:
        main()
