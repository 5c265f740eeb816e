"""BASELINE configs[3] in its stated form -- shards over several GPUs of one node with RCCL collectives over xGMI.
Runs whenever at least two GPUs are visible (the driver's 8-GPU node); skipped on a one-GPU box, where the same code
is covered by the world_size-2 gloo tests (tests/test_multigpu_cpu.py) and by G = 1 through the HIP kernels."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_commit_four_step_ntt_and_msm_over_rccl():
    from eigen_zeth_amd import native
    n = native.device_count()            # through the library, not torch (its wheel carries a second librccl: see tests/test_gpu_comm.py)
    if n < 2:
        pytest.skip("needs >= 2 GPUs (RCCL over xGMI); one visible")
    ranks = 4 if n >= 4 else 2           # at most 6 processes may hold the GPUs at once on the test box
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "multigpu_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["ok"] and res["world"] == ranks
    assert res["commit_root_matches_single_gpu"] and res["four_step_matches_plain_ntt"] and res["msm_matches_single_gpu"]
    assert res["sharded_proof_matches_single_gpu"]


def test_two_ranks_on_one_gpu_with_host_staged_collectives():
    """rehearsal on the one-GPU box: two processes, both computing on GPU 0 through the HIP kernels (pack / transpose / LDE /
    row-sharded Merkle / four-step NTT / MSM ranges / one sharded proof), collectives over gloo staged through the host --
    everything but the RCCL transport itself"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", ZP_CHECK_BACKEND="gloo", ZP_CHECK_LOGN="14", ZP_CHECK_STARK_LOGN="12")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "multigpu_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["ok"] and res["world"] == 2 and res["backend"] == "gloo"
    assert res["commit_root_matches_single_gpu"] and res["four_step_matches_plain_ntt"] and res["msm_matches_single_gpu"]
    assert res["sharded_proof_matches_single_gpu"]


def test_bench_n2_plain_launch_on_one_gpu():
    """`python3 bench.py --gpus 2 ...` typed PLAINLY -- no launcher, no WORLD_SIZE: the way the driver started the N = 1 run.  bench.py starts its
    two ranks itself (torch.distributed.run as a child, before anything touches the GPU), relays rank 0's ONE line and the ranks' exit code.
    Rehearsed on the one-GPU box with ZP_BENCH_BACKEND=gloo: the multi-rank pipeline probes (all-to-all commit, four-step NTT, MSM ranges,
    per-rank batch) run to completion, and the line says how many ranks the collective library delivered."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", ZP_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--logn", "20", "--cols", "16", "--stark-logn", "14",
           "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), "stdout of a plain launch is rank 0's single JSON line: %r" % r.stdout[-600:]
    line = json.loads(lines[0])
    # no --scaling flag, as the driver runs it: WEAK at every N since round 6 (independent columns, no data-path collective: every rank keeps --cols columns)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0 and line["config"]["cols_per_gpu"] == 16 and line["config"]["cols_total"] == 32
    assert line["rccl"]["ranks_seen_allreduce"] == 2 and line["rccl"]["world_env"] == 2 and line["rccl"]["self_launched"] and line["rccl"]["backend"] == "gloo"
    assert line["rccl"]["device_of_rank"] == [0, 0] or native_device_count() >= 2
    assert line["degraded"] is False and line["exchange_stalled"] is False
    pipe = line["pipeline"]
    assert "error" not in pipe and pipe["all_to_all_ms"] > 0 and pipe["four_step_single_column"]["ms"] > 0
    assert pipe["msm_bn254"]["on_curve"]
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "r6_bench_n2_plain_launch.json"), "w") as f:
            json.dump({"cmd": "ZP_BENCH_BACKEND=gloo python3 bench.py " + " ".join(cmd[2:]), "line": line}, f, indent=1)


def native_device_count():
    from eigen_zeth_amd import native
    return native.device_count()


def test_bench_strong_scaling_mode_and_the_timed_exchange_loops():
    """(i) bench.py --gpus 2 --scaling strong rehearsed over gloo: BASELINE configs[3] as stated -- `--cols` columns IN TOTAL, cols / N per
    GPU -- and the line says so; (ii) bench.py at N = 1 on RCCL: the exchange step of the path timed in its own K-step loops on the
    communicator behind the C-ABI (a communicator of one rank here: send / recv to self, all-gather, the code path a SCALE run takes)"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", ZP_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--logn", "18", "--cols", "16", "--scaling", "strong", "--no-pipeline", "--no-cpu"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["scaling"] == "strong" and line["config"]["cols_per_gpu"] == 8 and line["config"]["cols_total"] == 16 and line["n_gpus"] == 2
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--logn", "18", "--cols", "16", "--full", "--no-cpu",
           "--no-config5", "--stark-logn", "12"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    ex = line["pipeline"]["exchange"]
    assert "error" not in ex and ex["world"] == 1 and ex["all_to_all"]["steps"] == 3 and ex["all_to_all"]["median_ms"] > 0
    assert ex["sharded_commit"]["min_ms"] > 0 and ex["root_matches_torch_path"]
    # the communicator itself reports its size (ncclCommCount / ncclCommUserRank), and one commitment in the timed loop costs what the others do
    assert line["rccl"]["comm"] == {"transport": "rccl", "ranks_seen": 1, "user_rank": 0, "device": 0}
    assert line["degraded"] is False and line["exchange_stalled"] is False
    assert ex["sharded_commit"]["max_ms"] < 20 * ex["sharded_commit"]["median_ms"] + 50


def test_rccl_world_of_one_on_the_one_gpu_box():
    """RCCL itself on the driver's one-GPU box: tools/multigpu_check.py under torch.distributed.run with ONE rank and the
    `nccl` backend (= RCCL).  The process group is created on RCCL, and every collective wrapper of multigpu.py takes its
    device-tensor branch (all_to_all_single, all_gather, all_reduce, broadcast on HBM tensors -- no host staging): the
    column->row exchange + sharded commit, the four-step NTT, the MSM ranges and one sharded proof, each against the plain
    single-GPU result.  The child is launched before anything in this process touches the GPU."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", ZP_CHECK_BACKEND="nccl", ZP_CHECK_LOGN="14", ZP_CHECK_STARK_LOGN="12")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "multigpu_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["ok"] and res["world"] == 1 and res["backend"] == "nccl"
    assert res["commit_root_matches_single_gpu"] and res["four_step_matches_plain_ntt"] and res["msm_matches_single_gpu"]
    assert res["sharded_proof_matches_single_gpu"]


def test_engine_over_two_device_slots_keeps_witnesses_on_the_proving_gpu(tables, tmp_path):
    """Engine([f0, f1]): chunk i is uploaded through, and proven by, ctxs of device slot i % 2 (round 2 uploaded every
    witness through GPU 0 and handed the pointer to whichever ctx was free).  With >= 2 GPUs the slots are GPUs 0 and 1;
    on the one-GPU box both slots sit on GPU 0, which still exercises the per-slot uploaders and queues.  Proofs must equal
    the single-slot engine's byte for byte."""
    from eigen_zeth_amd import native
    from eigen_zeth_amd.service.engine import Engine, EngineConfig
    from eigen_zeth_amd.service.server import default_backend_factory
    second = 1 if native.device_count() >= 2 else 0
    mk = lambda: EngineConfig(air="chunk16", logn=12, chunks_per_block=1, crs_dir=str(tmp_path / "crs"), prover_streams=2)
    blocks = list(range(3, 10))                                        # 7 chunks: an odd count over two slots
    one = Engine(default_backend_factory(0), mk())
    ch = one.gen_batch_chunks("md", blocks, 12345, "evm")
    want = one.gen_chunk_proofs("md", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    two = Engine([default_backend_factory(0), default_backend_factory(second)], mk())
    got = two.gen_chunk_proofs("md", ch["task_id"], ch["chunk_count"], ch["batch_data"])
    assert [p["proof"] for p in got] == [p["proof"] for p in want]
    slots = two._free_be[2]
    assert len(slots) == 2 and slots[0].p_device == 0 and slots[1].p_device == second
