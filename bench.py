#!/usr/bin/env python3
"""bench.py -- headline metric of BASELINE.json on MI355X:  Goldilocks NTT field-elements/s at 2^24.

One step = one pass of the hot path over one batch: a natural-order forward NTT (zp_ntt through the
C-ABI) of the rank's column shard u64[cols][2^logn], resident in HBM before the timed region.
Columns are independent, so ranks shard columns with no data-path collective.  "scaling": "weak" (default): every GPU
always owns `--cols` columns.  --scaling strong: BASELINE configs[3] as stated -- `--cols` columns IN TOTAL, cols / N per GPU
(64 columns, 8 per GPU on 8 GPUs).  Rank 0 prints ONE JSON line.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--logn 24] [--cols 64] [--scaling weak|strong] [--dump-outputs DIR] [--full]
  N > 1 is launched by torch.distributed.run (one process per GPU, RCCL for the barrier/MAX only).

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step, ...).  Everything
below -- the exchange loops, the pipeline / batch-proof / configs[4] probes, the roofline, the size sweep and the CPU baselines --
runs only with --full (the --no-* options then leave parts of it out).  --dump-outputs DIR writes a fixed, seeded sample of what the
last timed step computed as float64 .npy files (dump_outputs()); the inputs are seeded, so two builds can be compared output for output.

The exchange step the path really has -- column shards -> row shards before leaf hashing, ONE all-to-all over xGMI -- is timed in its own
K-step loops ("pipeline.exchange": the bare all-to-all with GB/s per link, and the whole sharded commitment zp_merkle_commit_sharded;
median + min), on the RCCL communicator behind the C-ABI (a communicator of one rank at N = 1).

Extra objects on the line of a --full run: "roofline" (dominant kernel, HIP-event timing of every pass launch taken
live inside this run), "cpu_baseline" (oracle/ CPU restatement timed on this host, rank 0, N=1) and
"pipeline" (LDE + Poseidon Merkle commit of the same shard, timed outside the K steps).
The oracle is only used as the CPU baseline here, never in the measured path.
"""
import argparse
import json
import os
import sys
import threading
import time

# idle OpenMP workers of the CPU checker must sleep, not spin: spinning threads delay the host side of the GPU timings
# taken after the cpu_baseline leg (a DEEP launch measured 29 ms instead of 1.7 ms)
os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROBE_LIMIT_S = 300   # watchdog for the multi-rank probes of an N > 1 run
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s is the measured copy ceiling


def random_field_tensor(torch, shape, device, seed):
    """uniform 64-bit patterns reduced into [0,p): int64 storage of canonical u64 values"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    lo = torch.randint(0, 1 << 32, shape, dtype=torch.int64, device=device, generator=g)
    hi = torch.randint(0, 1 << 32, shape, dtype=torch.int64, device=device, generator=g)
    x = (hi << 32) | lo
    del lo, hi
    # unsigned x >= p  <=>  signed x in [-(2^32-1), -1]  -> subtract p == add 2^32-1 (mod 2^64)
    bad = (x < 0) & (x >= -((1 << 32) - 1))
    x = torch.where(bad, x + ((1 << 32) - 1), x)
    return x


DUMP_SAMPLE = 1 << 20   # output elements kept by --dump-outputs over all ranks: three float64 files of 8 MiB each


def dump_outputs(torch, x, directory, rank=0, world=1):
    """--dump-outputs: what the last timed step handed its caller -- the transformed columns, u64[cols][2^logn], in place in `x` -- as
    a fixed, seeded sample of DUMP_SAMPLE / world elements per rank (all of them when there are fewer), exact in float64:
      ntt_output_index  flat index column * 2^logn + row (sorted)
      ntt_output_hi     the upper 32 bits of the canonical value
      ntt_output_lo     the lower 32 bits
    At N > 1 every rank writes its own shard's files with a _rank<r> suffix."""
    import numpy as np
    total, keep = x.numel(), max(1, DUMP_SAMPLE // world)
    if total <= keep:
        idx = np.arange(total, dtype=np.int64)
    else:
        idx = np.unique(np.random.default_rng(0xD0B5 + rank).integers(0, total, size=keep, dtype=np.int64))
    vals = x.reshape(-1)[torch.from_numpy(idx).to(x.device)].cpu().numpy().view(np.uint64)
    tag = "_rank%d" % rank if world > 1 else ""
    os.makedirs(directory, exist_ok=True)
    for name, arr in (("ntt_output_index", idx), ("ntt_output_hi", vals >> np.uint64(32)), ("ntt_output_lo", vals & np.uint64(0xFFFFFFFF))):
        np.save(os.path.join(directory, name + tag + ".npy"), arr.astype(np.float64))


def host_cpu_info():
    """CPU model, physical cores (distinct (physical id, core id) pairs) and logical CPUs of this host, from /proc/cpuinfo"""
    model, pairs, logical, phys, core = "", set(), 0, None, None
    try:
        for line in open("/proc/cpuinfo"):
            if ":" not in line:
                if phys is not None or core is not None:
                    pairs.add((phys, core))
                phys = core = None
                continue
            k, v = [x.strip() for x in line.split(":", 1)]
            if k == "processor":
                logical += 1
            elif k == "model name" and not model:
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
        if phys is not None or core is not None:
            pairs.add((phys, core))
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 0
    return {"cpu_model": model, "physical_cores": len(pairs) or None, "logical_cpus": logical or None, "cpus_usable_by_this_process": usable,
            "cgroup_cpu_quota": cgroup_cpu_quota()}


def cgroup_cpu_quota():
    """CPUs' worth of CFS quota of this process's cgroup (None = unlimited / unknown): a container may SEE every CPU of
    the host and still be throttled to a few of them, which is what bounds an OpenMP baseline"""
    paths = ["/sys/fs/cgroup/cpu.max"]
    try:
        for line in open("/proc/self/cgroup"):
            rel = line.strip().split(":", 2)[-1]
            paths.insert(0, "/sys/fs/cgroup" + rel.rstrip("/") + "/cpu.max")
    except OSError:
        pass
    for pth in paths:
        try:
            q, per = open(pth).read().split()[:2]
            if q != "max":
                return float(q) / float(per)
        except (OSError, ValueError):
            continue
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return q / per
    except (OSError, ValueError):
        pass
    return None


def cpu_baseline(logn, budget_cols):
    """oracle NTT (OpenMP over columns) on a bounded sample of the same workload: one thread per physical core this
    process may use, plus the single-thread rate"""
    import numpy as np
    from oracle import oracle as O
    host = host_cpu_info()
    avail = O.num_threads()
    threads = max(1, min(avail, host["physical_cores"] or avail, host["cpus_usable_by_this_process"] or avail))
    if host["cgroup_cpu_quota"]:          # more threads than the quota only adds throttling
        threads = max(1, min(threads, int(host["cgroup_cpu_quota"] + 0.999)))
    x1 = O.random_field((1, 1 << logn), 0xE16E2E70 + 1)
    O.set_threads(1)
    t0 = time.perf_counter()
    y = O.ntt(x1)
    dt1 = time.perf_counter() - t0
    del y, x1
    # a bounded sample of about 10 s: whole rounds of one column per thread, at most 128 columns (16 GiB at 2^24)
    rounds = max(1, int(10.0 / max(dt1, 1e-3)))
    cols = max(1, min(threads * rounds, max(threads, 128) if threads <= 128 else threads))
    cols -= cols % threads if cols >= threads else 0
    O.set_threads(threads)
    x = O.random_field((cols, 1 << logn), 0xE16E2E70 + 2)
    t0 = time.perf_counter()
    y = O.ntt(x)
    dt = time.perf_counter() - t0
    del y
    O.set_threads(threads)    # later CPU legs (cpu_stark_baseline) keep the thread count the quota allows
    # subtract nothing: copy + transform is what the CPU path does per call
    return {"value": cols * (1 << logn) / dt, "unit": "field-elems/s", "cores": threads, "kind": "port",
            "sample": "%d columns x 2^%d rows, oracle/gl_oracle.c cache-blocked radix-2 NTT, OpenMP over columns, %d threads, %.2f s"
                      % (cols, logn, threads, dt),
            "single_thread_value": (1 << logn) / dt1, "effective_parallelism": round((cols * (1 << logn) / dt) / ((1 << logn) / dt1), 1), "host": host,
            "note": "CPU restatement, not the eigen-zkvm prover (parity unpinned, SURVEY.md 8c)"}


def integer_roofline(prover, pass_rows, alg_bytes, elems_per_launch, launches_per_step=None, ms_per_step=None):
    """the integer-VALU roofline next to the HBM one.  VALU instruction counts per element come from the committed PMC
    file (profiles/r6c_integer_roofline.json -- the newest of r6c / r6 / r5 --, made by tools/integer_roofline.py from a rocprofv3 --pmc SQ_INSTS_VALU run: labelled
    as such, not re-measured here; the counts equal the static ISA counts of profiles/r4_ntt_isa_breakdown.txt); the issue ceiling is
    1024 SIMDs x 64 lanes x clock / 4 cycles per instruction (every instruction of these kernels is of the 4-cycle class:
    tools/ubench_isa.hip, profiles/r2_ubench_isa.txt).  frac_int = the time the pure instruction issue of a launch needs / the
    measured launch time: a number in (0, 1] -- anything above 1 is a unit error in the table (round 4's file divided the count of a
    16-column launch by 8 columns), and the bench refuses to print it.  `plan` = the same over all launches of one step."""
    path = next((q for q in (os.path.join(ROOT, "profiles", f) for f in ("r6c_integer_roofline.json", "r6_integer_roofline.json", "r5_integer_roofline.json")) if os.path.exists(q)), None)
    try:
        if path is None:
            raise FileNotFoundError("profiles/r6_integer_roofline.json")
        tab = json.load(open(path))
        info = prover.device_info()
        clock = info["clock_khz"] * 1e3
        simds = info["cus"] * 4
        ceiling = simds * 64 * clock / tab.get("cycles_per_valu_instruction", 4.0)      # lane-instructions per second
        rows, plan_issue, plan_valu, covered = [], 0.0, 0.0, True
        for r in pass_rows:
            v = tab["ntt_valu_per_element_per_pass"].get(r["kernel"])
            if v is None or not r["avg_launch_ms"]:
                covered = False
                continue
            issue_ms = elems_per_launch * v / ceiling * 1e3
            frac = issue_ms / r["avg_launch_ms"]
            if not 0.0 < frac <= 1.0:
                raise ValueError("frac_int %.3f outside (0, 1] for %s: the VALU table's unit does not match the launch" % (frac, r["kernel"]))
            rows.append({"kernel": r["kernel"], "valu_per_element": v, "issue_only_ms": issue_ms, "measured_ms": r["avg_launch_ms"],
                         "frac_int": frac})
            plan_issue += issue_ms * (r["launches"] / float(launches_per_step[1]) if launches_per_step else 0.0)
            plan_valu += v
        plan = None
        if covered and launches_per_step and ms_per_step:
            # launches_per_step = (launches of ONE pass in a step, steps timed): issue-only time of a whole step
            plan = {"valu_per_element_all_passes": plan_valu, "issue_only_ms_per_step": plan_issue, "measured_ms_per_step": ms_per_step,
                    "frac_int": plan_issue / ms_per_step}
            if not 0.0 < plan["frac_int"] <= 1.0:
                raise ValueError("plan-level frac_int %.3f outside (0, 1]" % plan["frac_int"])
        return {"source": os.path.relpath(path, ROOT) + " (PMC SQ_INSTS_VALU x 64 / elements of the launch, separate profiler run)",
                "issue_ceiling_lane_instr_per_s": ceiling, "clock_hz": clock, "simds": simds,
                "cycles_per_valu_instruction": tab.get("cycles_per_valu_instruction", 4.0),
                "table_elements_per_launch_log2": tab.get("ntt_elements_per_launch_log2"),
                "ntt_passes": rows, "plan": plan, "other_stages_valu_per_unit": tab.get("stages", {})}
    except Exception as e:
        return {"error": repr(e)}


def ntt_roofline(prover, plan, passes, logn, cols, steps, dev_ms, copy_gbs):
    """--full: the `roofline` block of the line, from the per-launch events of the timed steps (set_profiling) and the committed PMC
    files: HBM fraction of every pass of the plan, the measured copy ceiling, the integer-VALU roofline"""
    N = 1 << logn
    npass = max(1, len(plan["passes"]))
    # Every launch of the timed region is one instantiation of ntt_pass2_kernel (one pass of the plan over chunk_cols
    # columns).  The roofline figure is TIME-WEIGHTED over all of them: algorithmic bytes of all launches / summed launch
    # time -- no instantiation is left out (round 2 reported the two cheaper ones only).  pass_timings() keys: radix log,
    # negative = the transposing first pass.
    by_kind, by_pass = {}, {}
    for j, (rl, ms) in enumerate(passes):
        by_kind.setdefault(rl, []).append(ms)
        by_pass.setdefault(j % npass, []).append(ms)       # launches are recorded in order: pass 0 .. npass-1 of every chunk of columns
    chunk_cols = min(cols, max(1, (1 << int(os.environ.get("ZP_NTT_CHUNK_LOG", "28"))) >> logn))
    # algorithmic bytes of one launch: SURVEY 8d gives 16*N bytes per column transform (ideal single
    # pass); a launch does one of the `npass` passes over chunk_cols columns -> 16*N*chunk/npass
    alg_bytes = 16.0 * N * chunk_cols / npass
    launches = sum(len(v) for v in by_kind.values())
    total_ms = sum(sum(v) for v in by_kind.values())
    avg_ms = total_ms / launches if launches else float("nan")
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if launches else float("nan")
    pass_rows = []
    for i, ps in enumerate(plan["passes"]):
        first, last = i == 0, i == len(plan["passes"]) - 1
        tw1 = first and plan.get("first_pass_table", False)
        mode = (3 if tw1 else 1) if first else (0 if last else 1)   # forward transform: table passes in the middle, plain last pass
        logt = {1: 0, 2: 1, 4: 2, 8: 3, 16: 4, 32: 5}[ps["tile"]]
        # <A1, A2, A3, LOGT, TRANSPOSE, PADDED, MODE, BIG, LIMB>: the canonical-arithmetic instantiations (knob ntt_limb = 0, the default)
        name = "ntt_pass2_kernel<%d, %d, %d, %d, %s, false, %d, false, false>" % (ps["rounds"][0], ps["rounds"][1], ps["rounds"][2], logt,
                                                                                    "true" if first else "false", mode)
        ms_l = by_pass.get(i, [])
        assert all(abs(rl) == ps["radix_log"] for rl, _ in passes[i::npass]), "pass timings out of step with the plan"
        a_ms = sum(ms_l) / len(ms_l) if ms_l else None
        pass_rows.append({"kernel": name, "role": ("transposing first pass (full twiddle table, shared by the columns through L2)" if tw1 else
                                                   "transposing first pass (per-lane twiddle chain)") if first else
                          ("plain last pass" if last else "pass with a per-tile twiddle table"),
                          "launches": len(ms_l), "avg_launch_ms": a_ms,
                          "frac": (alg_bytes / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if a_ms else None})
    slowest = max((r for r in pass_rows if r["avg_launch_ms"]), key=lambda r: r["avg_launch_ms"], default=None)
    traffic, traffic_src = None, None
    for tp in ("r6c_ntt_traffic.json", "r6_ntt_traffic.json", "r5_ntt_traffic.json", "r4_ntt_traffic.json"):
        tp = os.path.join(ROOT, "profiles", tp)
        if os.path.exists(tp):
            try:
                traffic = json.load(open(tp)).get("hbm_bytes_per_launch_dominant")
                traffic_src = ("committed PMC measurement %s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, FETCH x 2 "
                               "per the gfx950 correction); not re-measured in this run" % os.path.relpath(tp, ROOT))
                break
            except Exception:
                traffic = None
    integer = integer_roofline(prover, pass_rows, alg_bytes, N * chunk_cols, launches_per_step=(None, steps), ms_per_step=dev_ms / steps)
    return {
        "bound": "hbm",
        "kernel": "ntt_pass2_kernel: all %d instantiations of the plan, time-weighted (slowest: %s)" % (len(pass_rows), slowest["kernel"] if slowest else "?"),
        "passes": pass_rows,
        "launch_columns": chunk_cols,
        "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS if launches else None,
        "traffic": traffic, "traffic_source": traffic_src,
        "hbm_copy_ceiling_GBs": copy_gbs,
        "frac_of_copy_ceiling": (achieved / copy_gbs) if (launches and copy_gbs) else None,
        "algorithmic_bytes_per_launch": alg_bytes,
        "avg_launch_ms": avg_ms, "launches_timed": launches,
        "whole_transform_GBs": 16.0 * N * cols * steps / (dev_ms * 1e-3) / 1e9,
        "whole_transform_frac": 16.0 * N * cols * steps / (dev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "per_pass_avg_ms": {str(k): sum(v) / len(v) for k, v in sorted(by_kind.items())},
        "integer": integer,
    }


_REAL_STDOUT = [None]


def _quiet_stdout():
    """The contract is ONE JSON line on stdout.  Libraries loaded on the way print banners to the C-level stdout (RCCL: five lines of versions
    at the first communicator): from here on file descriptor 1 is stderr, and emit() writes the result line to the real stdout."""
    sys.stdout.flush()
    _REAL_STDOUT[0] = os.dup(1)
    os.dup2(2, 1)


def emit(line):
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)          # what C code buffered for stdout goes where fd 1 points now (stderr), not behind the result line
    except Exception:
        pass
    fd = _REAL_STDOUT[0] if _REAL_STDOUT[0] is not None else 1
    os.write(fd, (line + "\n").encode())


def self_launch(n, argv):
    """`python bench.py --gpus N` typed plainly (no launcher, no WORLD_SIZE): start the N ranks here -- `python -m torch.distributed.run`, one
    process per GPU, rendezvous on 127.0.0.1 at a free port -- as a CHILD of this process, which has not touched the GPU (nothing above imports
    torch or opens the library), relay rank 0's single JSON line to stdout and return the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, ZP_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    sys.stderr.write("bench.py: no WORLD_SIZE in the environment -- launching %d ranks: %s\n" % (n, " ".join(cmd)))
    sys.stderr.flush()
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    lines = 0
    for line in child.stdout:
        if line.startswith("{"):
            sys.stdout.write(line)
            sys.stdout.flush()
            lines += 1
        else:
            sys.stderr.write(line)
    rc = child.wait()
    if rc == 0 and lines != 1:
        sys.stderr.write("bench.py: the ranks exited 0 but printed %d result lines\n" % lines)
        rc = 4
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--logn", type=int, default=24)
    ap.add_argument("--cols", type=int, default=64, help="columns per GPU (--scaling weak) or in total (--scaling strong)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default=None,
                    help="weak: --cols columns per GPU; strong: --cols columns in total, cols / N per GPU (BASELINE configs[3]: 64 columns, 8 per GPU). "
                         "Default: WEAK at every N -- the columns of a trace are independent units with no data-path collective, every GPU keeps the 2^24 x 64 "
                         "workload the N = 1 line is quoted on (round 6; rounds 4-5 defaulted to strong with --gpus > 1: 8 columns = 1.4 ms per step and GPU "
                         "at N = 8, where launch and barrier overheads, not the kernel, set the figure)")
    ap.add_argument("--stark-logn", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--no-config5", action="store_true", help="skip the BASELINE configs[4]-on-one-GPU probe (64 chunks x 2^22 rows + the wrap's 2^26-point MSMs)")
    ap.add_argument("--c5-chunks", type=int, default=64)
    ap.add_argument("--c5-logn", type=int, default=22)
    ap.add_argument("--c5-msm-log", type=int, default=26)
    ap.add_argument("--stage-roofline", action="store_true",
                    help="cpu_baseline leg also times every hot-path stage on GPU and CPU restatement (tools/stage_roofline.py)")
    ap.add_argument("--full", action="store_true",
                    help="also run every probe, baseline and roofline figure beyond the headline (a plain run times the K steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a fixed seeded sample of the last step's output to DIR/<name>.npy (float64)")
    ap.add_argument("--child-probe", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.stage_roofline and not args.full:
        ap.error("--stage-roofline is part of the --full run")
    if not args.full:
        # the headline only: no probe, baseline or roofline outside the timed steps
        args.no_pipeline = args.no_cpu = args.no_config5 = True
    if args.scaling is None:
        args.scaling = "weak"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.child_probe:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    if not args.child_probe:
        _quiet_stdout()

    if args.child_probe:
        # the engine-level probe in a process of its own, as the service runs: WITHOUT torch.  With torch's CUDA context in the
        # process the library runs on the HIP runtime bundled with the torch wheel and the 8-stream batch measured 0.76 s
        # instead of 0.53 s (profiles/r2_pretorch.txt); torch is plumbing of this benchmark, not of the prover service.
        if args.child_probe.startswith("config5"):
            print(json.dumps(config5_probe(*[int(v) for v in args.child_probe.split(":")[1:]])), flush=True)
        else:
            print(json.dumps(batch_proof_probe(int(args.child_probe))), flush=True)
        return

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d (or plainly, without a launcher: bench.py starts its own ranks)"
                         % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no GPU visible (there is no CPU fallback)")
    # ZP_BENCH_BACKEND=gloo: rehearsal of the N > 1 code path with fewer GPUs than ranks (RCCL refuses two ranks on one
    # device): ranks compute on GPU local % device_count, collectives are staged through the host (eigen_zeth_amd/multigpu.py).
    # The driver's runs use the default, "nccl" (= RCCL).
    backend = os.environ.get("ZP_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    from eigen_zeth_amd import multigpu as MG

    # How many ranks did the TRANSPORT see?  WORLD_SIZE is what the launcher said; a sum of ones over the process group is what the collective
    # library delivered (RCCL at the default backend).  N worlds of one rank, or ranks that never joined, cannot produce N here.
    rccl_seen = {"backend": backend if world > 1 else "none (one rank)", "world_env": world, "ranks_seen_allreduce": 1,
                 "devices_visible": torch.cuda.device_count(), "self_launched": bool(os.environ.get("ZP_BENCH_SELF_LAUNCHED"))}
    if world > 1:
        ones = torch.ones(1, dtype=torch.int64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(ones)
        rccl_seen["ranks_seen_allreduce"] = int(ones.item())
        devs = torch.zeros(world, dtype=torch.int64, device=ones.device)
        devs[rank] = local + 1
        dist.all_reduce(devs)
        rccl_seen["device_of_rank"] = [int(v) - 1 for v in devs.tolist()]
        if rccl_seen["ranks_seen_allreduce"] != world:
            raise SystemExit("the process group delivered %d ranks, WORLD_SIZE says %d" % (rccl_seen["ranks_seen_allreduce"], world))

    from eigen_zeth_amd.native import Prover

    logn, cols = args.logn, args.cols
    if args.scaling == "strong":
        if cols % world:
            raise SystemExit("--scaling strong: %d columns do not split over %d GPUs" % (cols, world))
        cols //= world
    N = 1 << logn
    prover = Prover(local, stream=torch.cuda.current_stream().cuda_stream)
    if os.environ.get("ZP_NTT_TW1"):          # A/B knob: 0 = per-lane twiddle chains in the first pass instead of the full table
        prover.set_tuning("ntt_tw1", int(os.environ["ZP_NTT_TW1"]))
    if os.environ.get("ZP_NTT_CHUNK_LOG"):
        prover.set_tuning("ntt_chunk_log", int(os.environ["ZP_NTT_CHUNK_LOG"]))
    x = random_field_tensor(torch, (cols, N), dev, 0xE16E2E70 + 4 + rank)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        prover.ntt(x, x, logn, cols)
    barrier()
    prover.set_profiling(args.full)         # per-launch events for the roofline block (--full)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    step_ev[0].record()
    for k in range(args.steps):
        prover.ntt(x, x, logn, cols)
        step_ev[k + 1].record()
    ev1.record()
    barrier()
    wall = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    per_step = sorted(step_ev[k].elapsed_time(step_ev[k + 1]) for k in range(args.steps))   # median + min
    passes = prover.pass_timings() if args.full else []
    prover.set_profiling(False)
    if args.dump_outputs:
        # before anything below reuses the buffer (the sweep transforms its first columns in place)
        dump_outputs(torch, x, args.dump_outputs, rank, world)

    t = torch.tensor([wall], dtype=torch.float64, device=dev)
    if world > 1:
        MG.all_reduce(t, op=dist.ReduceOp.MAX)
    wall_max = float(t.item())

    # achievable HBM ceiling on this device (report against both the vendor peak and a measured copy):
    # device-to-device copy of the same 2^logn x cols matrix, read + write bytes counted
    copy_gbs = None
    if rank == 0 and args.full:
        y = torch.empty_like(x)
        ms = prover.hbm_copy_probe(x, y, x.numel() * 8, reps=5)     # libzethprover's own 16 B/lane non-temporal copy kernel
        copy_gbs = 2.0 * x.numel() * 8 / (ms * 1e-3) / 1e9
        del y

    # north_star: "Goldilocks NTT field-elems/s on synthetic 2^20-2^26 traces ... as absolute numbers and as fraction of HBM roofline" -- a compact live
    # sweep on the buffer of the timed region (16 columns; the full sweep with LDE and Merkle: tools/size_sweep.py -> profiles/r6_size_sweep.jsonl)
    sweep = None
    if rank == 0 and world == 1 and logn == 24 and cols >= 64 and args.full:
        try:
            sweep = []
            for lg in range(20, 27):
                v = x.view(-1)[:16 << lg].view(16, 1 << lg)
                prover.ntt(v, v, lg, 16)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 8 if lg <= 23 else 3
                e0.record()
                for _ in range(reps):
                    prover.ntt(v, v, lg, 16)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
                sweep.append({"logn": lg, "cols": 16, "passes": len(prover.ntt_plan(lg)["passes"]), "ms": ms, "Gelems_s": (16 << lg) / ms / 1e6,
                              "frac_hbm": 16.0 * (16 << lg) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
        except Exception as e:
            sweep = {"error": repr(e)}

    if rank == 0:
        plan = prover.ntt_plan(logn)
        elems_total = world * cols * N * args.steps
        out = {
            "metric": "goldilocks_ntt_field_elems_per_s",
            "value": elems_total / wall_max,
            "unit": "field-elems/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": wall_max * 1e3 / args.steps,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "full": args.full,            # false: the headline only; true: the probes, baselines and roofline below are on the line too
            "degraded": False,            # true: an optional probe failed or stalled; the K timed steps above are complete either way
            "exchange_stalled": False,    # true: a collective of the exchange probes never completed (watchdog) or returned an error
            "rccl": rccl_seen,
            "config": {"workload": ("forward NTT, natural order in/out, 2^%d rows x %d columns per GPU (column-major u64), "
                                    "BASELINE configs[3] shape on one GPU" % (logn, cols)) if args.scaling == "weak" else
                                   ("forward NTT, natural order in/out, 2^%d rows x %d columns in total, %d per GPU (column-major u64): BASELINE "
                                    "configs[3] as stated" % (logn, cols * world, cols)),
                       "logn": logn, "cols_per_gpu": cols, "cols_total": cols * world, "sharding": "columns, no data-path collective",
                       "plan": plan},
            "device_ms_per_step": dev_ms / args.steps,
            "device_ms_per_step_median": per_step[len(per_step) // 2],
            "device_ms_per_step_min": per_step[0],
        }
        if args.full:
            out["sweep"] = sweep
            out["roofline"] = ntt_roofline(prover, plan, passes, logn, cols, args.steps, dev_ms, copy_gbs)

    # ---- optional probes.  At N > 1 they contain collectives that cannot be rehearsed on the one-GPU development box:
    # a watchdog prints the line with the headline numbers and ends every rank if they do not return in time.
    out_lock = threading.Lock()
    printed = [False]
    watchdog = None
    wd_test = os.environ.get("ZP_BENCH_WATCHDOG_TEST")   # rehearsal hook: arm the watchdog on one GPU and stall the probes
    if (world > 1 and not args.no_pipeline) or wd_test:
        def bail():
            with out_lock:
                if rank == 0 and not printed[0]:
                    out["pipeline"] = {"error": "multi-rank probes did not finish within %d s; line printed by the watchdog" % PROBE_LIMIT_S}
                    out["degraded"] = out["exchange_stalled"] = True
                    emit(json.dumps(out))
                    printed[0] = True
            # The contract's line -- K timed steps of the hot path, no collective inside -- is complete and printed; what stalled is an OPTIONAL
            # probe, and the line says so at its top level ("degraded": true, "exchange_stalled": true) and in "pipeline".  Exit code 0: a
            # launcher that discards the output of a failed rank would lose the measured headline with it (ZP_BENCH_WATCHDOG_EXIT overrides:
            # the rehearsal test asks for 3).
            os._exit(int(os.environ.get("ZP_BENCH_WATCHDOG_EXIT", "0")))
        watchdog = threading.Timer(2 if wd_test else PROBE_LIMIT_S, bail)
        watchdog.daemon = True
        watchdog.start()
        if wd_test:
            time.sleep(6)

    pipe = None
    if not args.no_pipeline:
        del x
        torch.cuda.empty_cache()
        try:   # every rank takes part (all-to-all); reported by rank 0, outside the K timed steps
            pipe = pipeline_probe(torch, dist, prover, dev, logn, min(cols, 32), world, args.steps)
        except Exception as e:
            pipe = {"error": repr(e)}

    batch_multi = None
    if world > 1 and not args.no_pipeline:
        # BASELINE metric (i) on N GPUs: independent chunk proofs shard over the ranks with no exchange; every rank
        # proves its own 16-chunk batch (weak scaling) and the slowest rank's wall-clock is reported
        try:
            r = engine_batch_probe(16, args.stark_logn, "chunk64", device=local, tag="_r%d" % rank)
            tb = torch.tensor([r["wall_s"]], dtype=torch.float64, device=dev)
            err = None
        except Exception as e:
            tb = torch.tensor([-1.0], dtype=torch.float64, device=dev)
            err = repr(e)
        MG.all_reduce(tb, op=dist.ReduceOp.MAX)
        batch_multi = {"chunks_total": 16 * world, "chunks_per_gpu": 16, "wall_s_max_over_ranks": float(tb.item()),
                       "rank0_error": err}

    if watchdog is not None:
        watchdog.cancel()
    if rank == 0:
        extra = {}      # gathered outside the lock; merged into `out` and printed under it (the watchdog reads `out`)
        if pipe is not None:
            extra["pipeline"] = pipe
        if batch_multi is not None:
            extra["batch_proof"] = {"batch": batch_multi}
        if world == 1 and not args.no_pipeline:
            try:
                import subprocess
                torch.cuda.empty_cache()
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-probe", str(args.stark_logn)], capture_output=True,
                                   text=True, timeout=900)
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if r.returncode != 0 or not lines:
                    raise RuntimeError("child probe failed: " + (r.stderr or r.stdout)[-400:])
                extra["batch_proof"] = json.loads(lines[-1])
                extra["batch_proof"]["process"] = "child process without torch (the service's configuration)"
            except Exception as e:
                extra["batch_proof"] = {"error": repr(e)}
            if not args.no_config5:
                # BASELINE configs[4] on ONE GPU: 64 chunks x 2^22 rows x (64 + 12) columns, recursion, the wrap's MSM sizes
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-probe", "config5:%d:%d:%d" % (args.c5_chunks, args.c5_logn, args.c5_msm_log)],
                                       capture_output=True, text=True, timeout=1500)
                    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                    if r.returncode != 0 or not lines:
                        raise RuntimeError("config5 probe failed: " + (r.stderr or r.stdout)[-600:])
                    extra["batch_proof"]["config5_one_gpu"] = json.loads(lines[-1])
                except Exception as e:
                    extra["batch_proof"]["config5_one_gpu"] = {"error": repr(e)}
        if world == 1 and not args.no_cpu:
            extra["cpu_baseline"] = cpu_baseline(logn, 32)
            try:
                extra["cpu_baseline"]["stark"] = cpu_stark_baseline(min(args.stark_logn, 17))
            except Exception as e:
                extra["cpu_baseline"]["stark"] = {"error": repr(e)}
            if args.stage_roofline:
                try:
                    import types
                    from oracle import oracle as O, naive_bn254 as B1
                    from oracle.stark_cpu import CpuBackend
                    from tools import stage_roofline
                    extra["cpu_baseline"]["stages"] = stage_roofline.run(22, 32, cpu=types.SimpleNamespace(O=O, CpuBackend=CpuBackend, B1=B1))
                except Exception as e:
                    extra["cpu_baseline"]["stages"] = {"error": repr(e)}
        elif args.full:
            extra["cpu_baseline"] = None
        with out_lock:
            if not printed[0]:
                out.update(extra)
                pl = out.get("pipeline") or {}
                stalled = [k for k in ("exchange", "rccl_direct", "four_step_single_column") if isinstance(pl.get(k), dict) and pl[k].get("error")]
                if "error" in pl or stalled:
                    out["degraded"] = True
                    out["exchange_stalled"] = bool(stalled) or "error" in pl
                if isinstance(pl.get("rccl_direct"), dict) and pl["rccl_direct"].get("comm_info"):
                    out["rccl"]["comm"] = pl["rccl_direct"]["comm_info"]       # ncclCommCount / ncclCommUserRank of the C-ABI communicator
                for k in ("batch_proof",):
                    if isinstance(out.get(k), dict) and out[k].get("error"):
                        out["degraded"] = True
                emit(json.dumps(out))
                printed[0] = True
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "steps": len(ms)}


def exchange_probe(torch, comm, prover, y, M, cols, world, steps, barrier):
    """THE exchange step of the path, timed like the headline: `steps` timed repetitions after 2 warm-ups, barrier before each, wall-clock per
    call (a collective of this library returns when it is complete on the stream), median / min / max.
      all_to_all        the packed column shards [G][cols][M/G] through zp_comm_all_to_all (grouped ncclSend/ncclRecv: every pairwise message on
                        its own xGMI link): per-peer message = 8 cols M / G bytes; GB/s per link = that / time
      sharded_commit    zp_merkle_commit_sharded: pack + all-to-all + local subtree over M/G rows of all G cols columns + all-gather of sub-roots
    At N = 1 the communicator has one rank (send / recv to self): the code path, not xGMI."""
    dev = y.device
    Mloc = M // world
    words_per_peer = cols * Mloc
    pack = torch.empty((cols * M,), dtype=torch.int64, device=dev)
    rows = torch.empty((cols * M,), dtype=torch.int64, device=dev)
    tl = torch.empty(((2 * Mloc - 1) * 4,), dtype=torch.int64, device=dev)
    prover.pack_blocks(y, pack, cols, M, world) if world > 1 else pack.copy_(y.reshape(-1))
    a2a, com, root = [], [], None
    for it in range(steps + 2):
        barrier()
        t0 = time.perf_counter()
        comm.all_to_all(pack, rows, words_per_peer)
        torch.cuda.synchronize()
        if it >= 2:
            a2a.append((time.perf_counter() - t0) * 1e3)
    for it in range(steps + 2):
        barrier()
        t0 = time.perf_counter()
        root = comm.merkle_commit_sharded(y, M, cols, tl)
        torch.cuda.synchronize()
        if it >= 2:
            com.append((time.perf_counter() - t0) * 1e3)
    per_peer = 8.0 * words_per_peer
    st = _stats(a2a)
    res = {"world": world, "rows": M, "cols_per_gpu": cols,
           "all_to_all": dict(st, per_peer_message_bytes=per_peer, GBs_per_link_median=per_peer / (st["median_ms"] * 1e-3) / 1e9,
                              GBs_per_link_best=per_peer / (st["min_ms"] * 1e-3) / 1e9,
                              GBs_out_per_gpu_median=(world - 1) * per_peer / (st["median_ms"] * 1e-3) / 1e9,
                              xgmi_link_peak_GBs_bidirectional=153.0,
                              note="per-rank wall-clock around zp_comm_all_to_all; at N = 1 a copy to self, not a link"),
           "sharded_commit": dict(_stats(com), root=[hex(v) for v in root])}
    del pack, rows, tl
    return res


def pipeline_probe(torch, dist, prover, dev, logn, cols, world, steps=10):
    """commit stage of one trace shard: LDE (blow-up 2) of this rank's columns, then -- for N > 1 -- the
    column->row all-to-all over xGMI (eigen_zeth_amd/multigpu.py), then Poseidon leaf hashing + Merkle
    subtree of the local rows and the all-gather of sub-roots.  Timed once after one warm-up."""
    import numpy as np
    from eigen_zeth_amd import multigpu
    N = 1 << logn
    M = 2 * N
    multigpu.use_device_layout(prover)     # pack / transpose through zp_pack_blocks / zp_transpose on the ctx stream
    x = random_field_tensor(torch, (cols, N), dev, 99)
    y = torch.empty((cols, M), dtype=torch.int64, device=dev)
    Wtot, Mloc = cols * world, M // world
    tree = torch.empty(((2 * Mloc - 1) * 4,), dtype=torch.int64, device=dev)
    st = torch.zeros((12,), dtype=torch.int64, device=dev)

    def commit_rows(mat):
        prover.merkle_commit(mat, Mloc, Wtot, tree)
        return [int(v) & 0xFFFFFFFFFFFFFFFF for v in tree[-4:].tolist()]

    def hash_pair(l, r):
        vals = [v - (1 << 64) if v >= (1 << 63) else v for v in (list(l) + list(r) + [0] * 4)]
        st.copy_(torch.tensor(vals, dtype=torch.int64))
        prover.poseidon_perm(st, 1)
        return [int(v) & 0xFFFFFFFFFFFFFFFF for v in st[:4].tolist()]

    res = {}
    for it in range(2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        prover.lde(x, y, logn, 1, cols)
        e[1].record()
        if world > 1:
            rows, sent = multigpu.exchange_columns_to_rows(y)
        else:
            rows, sent = y, 0
        e[2].record()
        sub = commit_rows(rows)
        e[3].record()
        torch.cuda.synchronize()
        if world > 1:
            t = torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in sub], dtype=torch.int64, device=dev)
            allr = [torch.empty_like(t) for _ in range(world)]
            multigpu.all_gather(allr, t)
            root = multigpu.tree_top([[int(v) & 0xFFFFFFFFFFFFFFFF for v in r.tolist()] for r in allr], hash_pair)
        else:
            root = sub
        res = {"cols_per_gpu": cols, "blowup": 2, "lde_ms": e[0].elapsed_time(e[1]),
               "all_to_all_ms": e[1].elapsed_time(e[2]) if world > 1 else 0.0,
               "merkle_ms": e[2].elapsed_time(e[3]), "root": [hex(v) for v in root]}
        if world > 1:
            res["all_to_all_GBs_sent_per_gpu"] = sent / (res["all_to_all_ms"] * 1e-3) / 1e9
    # the same sharded commitment with RCCL called DIRECTLY behind the C-ABI (csrc/comm.hip: zp_comm_create on an id made by rank
    # 0, zp_merkle_commit_sharded = pack + grouped send/recv all-to-all + local subtree + all-gather of sub-roots + tree top) --
    # what a compiled host uses; must give the root of the torch.distributed path above.  RCCL wants one rank per GPU, so the
    # one-GPU rehearsal (gloo backend) skips it.
    direct_comm, grp1 = None, None
    if (world > 1 and dist.get_backend() == "nccl") or (world == 1 and os.environ.get("ZP_BENCH_BACKEND", "nccl") == "nccl"):
        try:
            from eigen_zeth_amd import native as _nat
            rk = dist.get_rank() if world > 1 else 0
            msg = torch.zeros(129, dtype=torch.int64, device=dev)
            if rk == 0:
                try:
                    msg[1:] = torch.tensor(list(_nat.comm_unique_id()), dtype=torch.int64)
                    msg[0] = 1
                except Exception:
                    pass
            if world > 1:
                multigpu.broadcast(msg, 0)
            if int(msg[0].item()) == 1:
                comm = _nat.Comm(prover, rk, world, bytes(int(v) for v in msg[1:].tolist()))
                comm.set_timeout_ms(60000)          # a peer that never arrives ends the probe with an error instead of the watchdog
                comm_info = comm.info()             # what RCCL itself reports: ranks in the communicator, this rank, its device
                tl = torch.empty(((2 * Mloc - 1) * 4,), dtype=torch.int64, device=dev)
                for it in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r2 = comm.merkle_commit_sharded(y, M, cols, tl)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                res["rccl_direct"] = {"comm_info": comm_info, "sharded_commit_ms": dt * 1e3, "root_matches_torch_path": [hex(v) for v in r2] == res["root"],
                                      "note": "zp_merkle_commit_sharded: exchange + hashing in one C-ABI call, wall-clock"}
                del tl

                def _barrier():
                    torch.cuda.synchronize()
                    if world > 1:
                        dist.barrier()
                try:
                    res["exchange"] = exchange_probe(torch, comm, prover, y, M, cols, world, steps, _barrier)
                    res["exchange"]["root_matches_torch_path"] = res["exchange"]["sharded_commit"]["root"] == res["root"]
                except Exception as ex:
                    res["exchange"] = {"error": repr(ex)}
                direct_comm = comm            # kept for the four-step NTT below, closed there
            else:
                res["rccl_direct"] = {"error": "rank 0 could not make an RCCL id"}
        except Exception as ex:
            res["rccl_direct"] = {"error": repr(ex)}
    # one column of 2^28 elements split over the ranks (SURVEY 8e alternative): four-step NTT, three transposes
    try:
        flog = 28
        ops = multigpu.hip_row_ops(prover)
        blk = random_field_tensor(torch, ((1 << flog) // world,), dev, 7 + (dist.get_rank() if world > 1 else 0))
        for it in range(2):
            f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f0.record()
            multigpu.four_step_ntt(blk, flog, *ops)
            f1.record()
            torch.cuda.synchronize()
        res["four_step_single_column"] = {"logn": flog, "ms": f0.elapsed_time(f1),
                                          "elems_per_s": (1 << flog) / (f0.elapsed_time(f1) * 1e-3)}
        # the same transform behind ONE C-ABI call per rank (zp_ntt_sharded: RCCL all-to-all per transpose; at N = 1 a
        # communicator of one rank, the transposes are local) -- must give the torch.distributed result, element for element
        if direct_comm is None and world == 1:
            from eigen_zeth_amd import native as _nat
            grp1 = _nat.CommGroup(1)
            direct_comm = _nat.Comm(prover, 0, 1, group=grp1)
        run_direct = direct_comm is not None
        if world > 1:       # every rank or none: a rank whose communicator failed must not leave the others in a collective
            flag = torch.tensor([1 if run_direct else 0], dtype=torch.int64, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            run_direct = bool(int(flag.item()))
        if run_direct:
            want = multigpu.four_step_ntt(blk, flog, *ops)
            tmp = torch.empty((2 * blk.numel(),), dtype=torch.int64, device=dev)
            for it in range(2):
                d = blk.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                direct_comm.ntt_sharded(d, tmp, flog)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            res["four_step_single_column"]["c_abi"] = {"ms": dt * 1e3, "elems_per_s": (1 << flog) / dt, "equals_torch_path": bool(torch.equal(d, want)),
                                                       "note": "zp_ntt_sharded, wall-clock incl. the copy back to the caller's buffer"}
            del want, tmp, d
        del blk
    except Exception as ex:
        res["four_step_single_column"] = {"error": repr(ex)}
    if direct_comm is not None:
        try:
            direct_comm.close()
            if grp1 is not None:
                grp1.close()
        except Exception:
            pass
    # BN254 MSM over the ranks: 2^22 points per GPU, partial sums all-gathered and added
    try:
        from eigen_zeth_amd.service import bn254
        from eigen_zeth_amd import native as _native
        rk = dist.get_rank() if world > 1 else 0
        g = np.random.default_rng(100 + rk)
        nloc = 1 << 22
        pts = _native.synth_g1_points(nloc, start=1025 + rk * nloc)     # all ranks' points distinct: (1025 + i) G
        scs = g.integers(0, 1 << 32, size=(nloc, 8), dtype=np.uint64).astype(np.uint32)
        scs[:, 7] &= 0x1FFFFFFF
        add = lambda p, q: bn254._pt_add(bn254._Ops1, p, q)
        multigpu.distributed_msm(lambda: prover.msm_bn254_arrays(pts, scs), add)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = multigpu.distributed_msm(lambda: prover.msm_bn254_arrays(pts, scs), add)
        dt = time.perf_counter() - t0
        res["msm_bn254"] = {"points_per_gpu": nloc, "points": "distinct: (1025 + i) G (zp_synth_g1_points), uniform 253-bit scalars",
                            "wall_ms_incl_upload": dt * 1e3, "points_per_s_all_gpus": world * nloc / dt,
                            "on_curve": bool(total is None or bn254.g1_on_curve(total))}
    except Exception as ex:
        res["msm_bn254"] = {"error": repr(ex)}
    perms = ((Wtot + 7) // 8) * Mloc + (Mloc - 1)
    # lde_ms is the extension AS THE PROVERS ISSUE IT since round 5 (csrc/prove.hip, stark/backend_hip.py: no coefficient store, the
    # out-of-domain evaluations read the extension -- zp_ood_eval); the form that also stores the scaled coefficients (what rounds 1-4's
    # provers called) is timed beside it under its own label
    res["lde_form"] = "zp_lde without a coefficient store = the prover's call (round 5); path: %s" % json.dumps(prover.ntt_plan(logn).get("lde"))
    res["lde_GBs_algorithmic"] = 8.0 * N * 3 * cols / (res["lde_ms"] * 1e-3) / 1e9
    try:
        coef = torch.empty((cols, N), dtype=torch.int64, device=dev)
        prover.lde(x, y, logn, 1, cols, d_coef=coef)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        prover.lde(x, y, logn, 1, cols, d_coef=coef)
        e1.record()
        torch.cuda.synchronize()
        res["lde_with_coefficient_store_ms"] = e0.elapsed_time(e1)
        del coef
    except Exception as ex:
        res["lde_with_coefficient_store_ms"] = repr(ex)
    res["poseidon_perms_per_s_per_gpu"] = perms / (res["merkle_ms"] * 1e-3)
    return res


def batch_proof_probe(logn, air_name="chunk64"):
    """BASELINE configs[2]-shaped: one chunk, full STARK (trace -> LDE -> constraints -> FRI) on one GPU"""
    from eigen_zeth_amd import native
    from eigen_zeth_amd.stark import air as AIR, prover as PR
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    air = AIR.get_air(air_name)
    t0 = time.perf_counter()
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 42)
    tw = time.perf_counter() - t0
    be = HipBackend(0)
    params = PR.StarkParams(logn, logb=1, fri_logf=3, fri_final_log=5, n_queries=80, pow_bits=20)   # the service default: 100 bits
    PR.prove(air, tr, pub, params, be)
    tm = {}
    t0 = time.perf_counter()
    proof = PR.prove(air, tr, pub, params, be, timings=tm)
    wall = time.perf_counter() - t0
    out = {"workload": "single chunk full STARK, AIR %s (%d columns), 2^%d rows, blow-up 2, 80 queries + 20 grinding bits (%d bits conjectured)"
                       % (air_name, air.width, logn, params.security_bits()),
           "wall_s": wall, "stages_ms": {k: round(v * 1e3, 2) for k, v in tm.items()},
           "witness_host_s": tw, "proof_bytes": len(PR.proof_to_json(proof))}
    try:      # the same proof through the one-call prover (zp_stark_prove): what the engine uses per chunk
        be.prove_native(air, tr, pub, params)
        t0 = time.perf_counter()
        text = be.prove_native(air, tr, pub, params)
        out["one_call_prover"] = {"wall_s": time.perf_counter() - t0, "same_proof_text": text == PR.proof_to_json(proof),
                                  "note": "zp_stark_prove: witness upload + the whole STARK in one C-ABI call (constraints through the program interpreter)"}
        # ... and with the trace already in HBM when the clock starts (what zp_stark_prove itself takes: a device pointer; the batch pipeline
        # uploads chunk k + 1 while chunk k is proven): the upload of 2^logn x W words over one PCIe link is the difference
        res = []
        for _ in range(3):
            d_tr = be.p.upload(tr)
            be.p.sync()
            t0 = time.perf_counter()
            text2 = be.prove_native(air, d_tr, pub, params)
            res.append(time.perf_counter() - t0)
        out["one_call_prover"]["wall_s_trace_resident"] = sorted(res)[1]
        out["one_call_prover"]["same_proof_text_trace_resident"] = text2 == text
    except Exception as e:
        out["one_call_prover"] = {"error": repr(e)}
    del be, tr
    try:   # BASELINE metric (i): batch-proof wall-clock, GenBatchChunks -> GenFinalProof, through the engine
        out["batch"] = engine_batch_probe(16, logn, air_name)
    except Exception as e:
        out["batch"] = {"error": repr(e)}
    try:   # ... and REQUEST TO RESPONSE over the wire: the gRPC service + the mirror of eigen-zeth's client state machine
        out["grpc_request_to_response"] = grpc_probe(logn, air_name)
    except Exception as e:
        out["grpc_request_to_response"] = {"error": repr(e)}
    return out


def grpc_probe(logn, air_name, chunks_per_block=8, blocks=3):
    """BASELINE metric (i) as the reference's client sees it: ProverChannel.execute(block) = GenBatchChunks -> GenChunkProof ->
    GenAggregatedProof -> GenFinalProof over one bidi stream (src/prover/provider.rs:243-544, without its 1-s sleeps) against the
    service on this GPU; one block of `chunks_per_block` chunks; the last of `blocks` blocks is reported (the first builds the CRS
    and warms the pools).  The synthetic witness generator (host code) is inside, as it is in the service."""
    import tempfile
    from eigen_zeth_amd.service.client import ProverChannel
    from eigen_zeth_amd.service.engine import EngineConfig
    from eigen_zeth_amd.service.server import serve
    tmp = tempfile.mkdtemp()
    cfg = EngineConfig(air=air_name, logn=logn, chunks_per_block=chunks_per_block, crs_dir=os.path.join(tmp, "crs"), witness_threads=16)
    server, port = serve(0, "127.0.0.1", os.path.join(tmp, "state"), cfg, 0)
    try:
        ch = ProverChannel("127.0.0.1:%d" % port)
        walls = []
        for b in range(1, blocks + 1):
            t0 = time.perf_counter()
            res = ch.execute(b)
            walls.append(time.perf_counter() - t0)
        ch.close()
        return {"wall_s": walls[-1], "all_blocks_wall_s": [round(w, 3) for w in walls], "chunks_per_block": chunks_per_block,
                "chunk_rows_log2": logn, "proof_bytes": len(res["proof"]),
                "note": "one block = %d chunk STARKs + aggregation STARK + final STARK (BN128) + Groth16 wrap, request to response over gRPC" % chunks_per_block}
    finally:
        server.stop(0)


def engine_batch_probe(K, logn, air_name, device=0, tag=""):
    """K blocks -> K chunk STARKs -> aggregate -> Groth16 wrap on one GPU through service/engine.py (no gRPC), at the
    service's default security (80 queries, blow-up 2, 20 grinding bits).  Reported twice: with the synthetic witness
    generator (host code standing in for the zkVM executor) inside the timed region, and with the witnesses generated
    beforehand (what the prover itself costs).  Each is the last of two / three runs (the first builds the local CRS and
    warms the buffer pools)."""
    import tempfile
    from eigen_zeth_amd.service.engine import Engine, EngineConfig
    from eigen_zeth_amd.service.server import default_backend_factory
    cfg = EngineConfig(air=air_name, logn=logn,
                       crs_dir=os.path.join(tempfile.gettempdir(), "zp_crs_bench_%d%s" % (os.getuid(), tag)), witness_threads=16)
    eng = Engine(default_backend_factory(device), cfg)
    eng.groth16_keys()
    res = {}
    for pre in (False, True):
        eng.pregenerate_witnesses = pre
        for rep in range(3 if pre else 2):     # steady state: the first runs build the CRS and fill the buffer pools of every stream
            ch = eng.gen_batch_chunks("bench", list(range(1, K + 1)), 12345, "evm")
            tw0 = time.perf_counter()
            if pre:
                eng.prepare_witnesses(ch["batch_data"])
            t0 = time.perf_counter()
            proofs = eng.gen_chunk_proofs("bench", ch["task_id"], ch["chunk_count"], ch["batch_data"])
            t1 = time.perf_counter()
            agg = eng.aggregate("bench", proofs[0]["proof"], proofs[-1]["proof"])
            eng.final("bench", agg, "BN128", "479881985774944702531460751064278034642760119942")
            t2 = time.perf_counter()
            r = {"wall_s": t2 - t0, "chunk_proofs_s": t1 - t0, "aggregate_final_s": t2 - t1,
                 "aggregate_stages_s": {k: round(v, 4) for k, v in eng.stage_timings.get("aggregate/bench", {}).items()},
                 "final_stages_s": {k: round(v, 4) for k, v in eng.stage_timings.get("final/bench", {}).items()}}
            if pre:
                r["witness_generation_s_outside"] = t0 - tw0
        res["witnesses_pregenerated" if pre else "with_witness_generator"] = r
    res.update({"chunks": K, "prover_streams": cfg.prover_streams, "wall_s": res["witnesses_pregenerated"]["wall_s"],
                "groth16_wrap": getattr(eng, "wrap_info", None),
                "stark_security_bits": eng.stark_params(logn).security_bits(),
                "note": "wall_s = prover only (witnesses pre-generated); the synthetic generator is host code (about 0.2 s per 2^20 x 64 chunk)"})
    return res


def config5_probe(K=64, logn=22, msm_log=26, air_name="chunk64"):
    """BASELINE configs[4] on ONE GPU (64 chunk-sized STARKs as C3 -- 2^22 rows x 64 + 12 columns -- + the Groth16 wrap's
    2^26-point MSMs), through service/engine.py as the service runs it (no gRPC, no torch), at the service's default security:
      chunk proofs        K x zp_stark_prove on 8 streams, witnesses from the synthetic generator (host code standing in for the executor)
      recursion           the client's contract: GenAggregatedProof(first, last) -> GenFinalProof (final STARK in BN128-hash mode + wrap);
                          and the fold of ALL K chunk proofs as a binary tree of GenAggregatedProof calls (K - 1 aggregation STARKs) under one
                          final proof -- what a batch-covering proof costs with this prover's pairwise aggregation
      the wrap's MSMs     round 6: the wrap verifies the final STARK's hashing AND its field arithmetic (stage B-2): 3.2 M constraints, a 2^22 QAP
                          domain, MSMs of 2.8 M - 4.2 M points ON THE REQUEST PATH, inside final_s (batch.groth16_wrap, final_stages_s); the
                          2^msm_log-point size BASELINE names is timed beside it on synthetic points, labelled
    One warm-up batch of 8 chunks first (CRS, buffer pools, plan tables)."""
    import ctypes as C
    import random
    import tempfile
    import numpy as np
    from eigen_zeth_amd.native import DeviceBuffer
    from eigen_zeth_amd.service import bn254
    from eigen_zeth_amd.service.engine import Engine, EngineConfig
    from eigen_zeth_amd.service.server import default_backend_factory
    cfg = EngineConfig(air=air_name, logn=logn, crs_dir=os.path.join(tempfile.gettempdir(), "zp_crs_c5_%d" % os.getuid()),
                       witness_threads=int(os.environ.get("ZP_C5_WITNESS_THREADS", "12")),          # 2 GiB of page-locked witness per chunk in flight at 2^22 x 64 (14 in flight at most)
                       prover_streams=int(os.environ.get("ZP_C5_STREAMS", "8")))                    # (both overridable for sweeps: tools, not the driver's run)
    eng = Engine(default_backend_factory(0), cfg)
    eng.groth16_keys()
    out = {"workload": "%d chunks x 2^%d rows x (64 + 12) columns, %d bits conjectured; recursion; 4 G1 + 1 G2 MSMs of 2^%d points"
                       % (K, logn, eng.stark_params(logn).security_bits(), msm_log)}
    addr = "479881985774944702531460751064278034642760119942"

    def batch(n, label, tree):
        r = {}
        t0 = time.perf_counter()
        ch = eng.gen_batch_chunks(label, list(range(1, n + 1)), 12345, "evm")
        proofs = eng.gen_chunk_proofs(label, ch["task_id"], ch["chunk_count"], ch["batch_data"])
        t1 = time.perf_counter()
        agg = eng.aggregate(label, proofs[0]["proof"], proofs[-1]["proof"])
        t2 = time.perf_counter()
        eng.final(label, agg, "BN128", addr)
        t3 = time.perf_counter()
        wit = sum(v.get("witness(host)", 0.0) for k, v in eng.stage_timings.items() if k.startswith(ch["task_id"] + "/"))
        prv = sum(v.get("total", 0.0) for k, v in eng.stage_timings.items() if k.startswith(ch["task_id"] + "/"))
        r["groth16_wrap"] = getattr(eng, "wrap_info", None)
        r["final_stages_s"] = {k: round(v, 4) for k, v in eng.stage_timings.get("final/" + label, {}).items()}
        wdev = [v["witness(device)"] for k, v in eng.stage_timings.items() if k.startswith(ch["task_id"] + "/") and "witness(device)" in v]
        r["witness"] = {"mode": cfg.witness, "chunks_from_the_host_generator": n - len(wdev), "chunks_filled_in_hbm": len(wdev),
                        "fill_from_checkpoints_s_summed": sum(wdev),
                        "note": "device mode: the recurrences of the batch are walked once on the GPU (one wave per chunk, csrc/synth.hip) while the first "
                                "witness_threads chunks come from the host generator and are proven; the same traces word for word (tests/test_gpu_synth.py)"}
        r.update({"chunk_proofs_s": t1 - t0, "witness_generator_cpu_s_summed_over_threads": wit, "witness_threads": cfg.witness_threads,
                  "zp_stark_prove_s_summed_over_streams": prv, "prover_streams": cfg.prover_streams,
                  "aggregate_first_last_s": t2 - t1, "final_s": t3 - t2,
                  "wall_s": t3 - t0, "aggregated_proof_bytes": len(agg)})
        if tree and n >= 4:
            t0 = time.perf_counter()
            level = [p["proof"] for p in proofs]
            n_aggs = 0
            while len(level) > 1:
                nxt = []
                for i in range(0, len(level) - 1, 2):
                    nxt.append(eng.aggregate(label, level[i], level[i + 1]))
                    n_aggs += 1
                if len(level) % 2:
                    nxt.append(level[-1])
                level = nxt
            t1 = time.perf_counter()
            eng.final(label, level[0], "BN128", addr)
            t2 = time.perf_counter()
            r["fold_all_chunks"] = {"aggregation_starks": n_aggs, "fold_s": t1 - t0, "final_s": t2 - t1, "top_proof_bytes": len(level[0]),
                                    "wall_s_chunks_plus_fold_plus_final": r["chunk_proofs_s"] + (t2 - t0)}
        return r
    batch(8 if K >= 8 else K, "warm", False)
    out["batch"] = batch(K, "c5", True)
    out["wall_s"] = out["batch"]["wall_s"]
    # ---- the MSM sizes of a 2^26-constraint wrap, on the same GPU
    try:
        p = eng.be.p
        rnd, g = random.Random(3), np.random.default_rng(7)
        n, chunk = 1 << msm_log, 1 << min(msm_log, 20)
        t1 = np.array([[(c >> (32 * k)) & 0xFFFFFFFF for c in pt for k in range(8)] for pt in [bn254.g1_mul(rnd.randrange(1, bn254.R)) for _ in range(32)]],
                      dtype=np.uint32)
        t2 = np.array([[(c >> (32 * k)) & 0xFFFFFFFF for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) for k in range(8)]
                       for pt in [bn254.g2_mul(rnd.randrange(1, bn254.R)) for _ in range(16)]], dtype=np.uint32)
        scs = g.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        scs[:, 7] &= 0x1FFFFFFF
        d_s = DeviceBuffer(p, scs.size // 2)
        p._chk(p.lib.zp_h2d(p.ctx, d_s.ptr, scs.ctypes.data, scs.nbytes))
        del scs

        def tiled(tab, words):             # one 2^20-point slice from the host, replicated on the device
            sl = np.ascontiguousarray(tab[g.integers(0, len(tab), size=chunk)])
            d = DeviceBuffer(p, n * words // 2)
            p._chk(p.lib.zp_h2d(p.ctx, d.ptr, sl.ctypes.data, sl.nbytes))
            for i in range(1, n // chunk):
                p._chk(p.lib.zp_d2d(p.ctx, d.offset(i * chunk * words // 2), d.ptr, sl.nbytes))
            return d
        d_p1, d_p2 = tiled(t1, 16), tiled(t2, 32)
        o1, o2 = (C.c_uint32 * 16)(), (C.c_uint32 * 32)()
        p._chk(p.lib.zp_msm_bn254(p.ctx, d_p1.ptr, d_s.ptr, n, o1))
        ta = time.perf_counter()
        for _ in range(4):
            p._chk(p.lib.zp_msm_bn254(p.ctx, d_p1.ptr, d_s.ptr, n, o1))
        tb = time.perf_counter()
        # The G2 run needs a larger Pippenger arena than the G1 runs grew (points twice the size): its FIRST call pays a multi-GiB hipMalloc.
        # Rounds 3-4 timed exactly that first call -- 0.37 s on one box, 0.61 s on the driver's, the spread being the allocator, not the kernels
        # (round-4 review item).  The first call is now reported on its own and the steady-state call is the figure.
        p._chk(p.lib.zp_msm_bn254_g2(p.ctx, d_p2.ptr, d_s.ptr, n, o2))
        tg = time.perf_counter()
        p._chk(p.lib.zp_msm_bn254_g2(p.ctx, d_p2.ptr, d_s.ptr, n, o2))
        tc = time.perf_counter()
        out["wrap_msm_sizes"] = {"points": n, "g1_4x_s": tb - ta, "g2_1x_s": tc - tg, "g2_first_call_s_incl_arena_growth": tg - tb,
                                 "note": "synthetic points (a 2^20-point slice of a 32 / 16-point table, tiled) and uniform 253-bit scalars; NOT part of wall_s: "
                                         "the wrap circuit of this build (stage B-2) has 3.2 M constraints: its own MSMs of 2.8 - 4.2 M points are inside final_s"}
        out["wall_s_plus_wrap_msm_sizes"] = out["wall_s"] + (tb - ta) + (tc - tg)
        for d in (d_s, d_p1, d_p2):
            d.free()
    except Exception as e:
        out["wrap_msm_sizes"] = {"error": repr(e)}
    return out


def cpu_stark_baseline(logn, air_name="chunk64"):
    import numpy as np
    from eigen_zeth_amd import native
    from eigen_zeth_amd.poseidon_constants import default_round_constants, default_mds
    from eigen_zeth_amd.stark import air as AIR, prover as PR
    from oracle.stark_cpu import CpuBackend
    from oracle import oracle as O
    air = AIR.get_air(air_name)
    tr, pub = native.synth_trace(air.trace_kind, logn, air.width, 42)
    be = CpuBackend(default_round_constants(), default_mds())
    tm = {}
    t0 = time.perf_counter()
    params = PR.StarkParams(logn, 1, 3, 5, 80, pow_bits=20)        # the GPU line's parameters: 80 queries + 20 grinding bits
    PR.prove(air, tr, pub, params, be, timings=tm)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "cores": O.num_threads(), "kind": "port",
            "sample": "same STARK (same AIR, same parameters: 80 queries + 20 grinding bits) at 2^%d rows on the CPU restatement (oracle/stark_cpu.py); the GPU line is at 2^20" % logn,
            "extrapolated_2^20_wall_s": wall * (1 << (20 - logn)) if logn < 20 else wall,
            "extrapolation": "linear in the row count (every stage is O(N) or O(N log N)): a lower bound for the CPU at 2^20",
            "stages_ms": {k: round(v * 1e3, 1) for k, v in tm.items()}}


if __name__ == "__main__":
    main()
