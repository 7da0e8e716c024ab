"""The N > 1 launch path of bench.py on real hardware at world size 1: under torchrun RANK is set, so the worker takes the
`nccl` (= RCCL) init, the CUDA barrier and the all_reduce(MAX) / all_gather of the clock exactly as an 8-GPU run does
(bench.py main()).  One worker per request/GPU is the reference's concurrency model (proving-server/src/main.rs:457-472);
proofs are replicas, there is no data-path collective to test."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bench_under_torchrun_one_rank_nccl():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ZKMI355_BENCH_FAKE")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--k17-steps", "0", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["metric"] == "webauthn_es256_proofs_per_sec_k19" and j["n_gpus"] == 1 and j["steps"] == 2
    assert j["launcher"] == "torchrun" and j["dist_backend"] == "nccl"
    assert len(j["ms_per_step_per_rank"]) == 1 and abs(j["ms_per_step_per_rank"][0] - j["ms_per_step"]) < 1e-6  # (both of the K timed steps)
    assert j["value"] == j["value_first"] == j["value_repeats"][0] and j["value_median"] == sorted(j["value_repeats"])[2]
    assert j["config"]["proof_bytes"] == 960 and j["value"] > 1.0


def test_two_worker_processes_share_one_gpu():
    """The N > 1 path with REAL proofs across two processes (round 6): two ranks under torchrun, both on device 0 (`--one-device`),
    `gloo` for the barrier and the clocks (two ranks of one device cannot form an RCCL communicator; the `nccl` leg is the test
    above), 8 timed steps each.  What has never touched hardware before: two worker processes proving side by side on one device
    (two HIP runtimes, their contexts' streams on the same hardware queues), rank r proving jobs r, r + 2, ... and every one of the
    16 proofs compared with the oracle's committed digest; the ranks' jobs partition 0 .. 15.  The reference's model is one
    worker per request (proving-server/src/main.rs:457-472)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ZKMI355_BENCH_FAKE")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "1",
           "--inflight", "2", "--no-cpu-baseline", "--backend", "gloo", "--one-device", "--k17-steps", "0", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 8 and j["jobs_total"] == 16
    assert j["launcher"] == "torchrun" and j["dist_backend"] == "gloo"
    assert j["jobs_covered_exactly_once"] is True
    assert j["proofs_checked_against_oracle_digests"] == 16  # both ranks' timed proofs, byte-compared through their digests
    assert len(j["ms_per_step_per_rank"]) == 2 and all(t > 0 for t in j["ms_per_step_per_rank"])
    assert j["ranks_share_device"] is True
