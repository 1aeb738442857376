"""bench.py launch-contract rehearsal (what the driver runs at round end).

The driver launches `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...` — this
test runs that EXACT shape at N=8 on CPU/gloo (tiny model) and checks
the one-line JSON contract, plus the honest-n_gpus guard."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the rehearsals run the CPU/gloo engine on every machine: same ranks and
# same arrays whether the host has no GPU, one, or eight
CPU_ENV = {**os.environ, "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}


def test_torchrun_world8_bench_contract(tmp_path):
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29751", "bench.py", "--gpus", "8",
         "--model", "tiny-qwen3", "--steps", "4", "--warmup", "1",
         "--concurrency", "4", "--prompt-len", "48", "--gen-len", "6"],
        capture_output=True, text=True, timeout=420, cwd=REPO, env=CPU_ENV,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 8
    assert rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["scaling"] == "weak" and rec["dtype"] == "bf16"
    assert rec["config"]["parallelism"] == "dp8"
    assert rec["value"] > 0 and rec["higher_is_better"] is True


def test_bench_refuses_dishonest_gpus():
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "4", "--steps", "1"],
        capture_output=True, text=True, timeout=120, cwd=REPO,
    )
    assert out.returncode != 0
    assert "WORLD_SIZE=1" in out.stderr


def _tiny_cpu_bench(*extra):
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--model", "tiny-qwen3",
         "--steps", "6", "--warmup", "2", "--concurrency", "4",
         "--prompt-len", "48", "--gen-len", "6", *extra],
        capture_output=True, text=True, timeout=120, cwd=REPO, env=CPU_ENV,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last delivering timed step as float
    .npy arrays, identical from run to run; --steps sets the timed steps
    and the record carries ms_per_step."""
    a, b = tmp_path / "a", tmp_path / "b"
    rec = _tiny_cpu_bench("--dump-outputs", str(a))
    _tiny_cpu_bench("--dump-outputs", str(b), "--full")
    assert rec["steps"] == 6 and rec["warmup"] == 2
    assert rec["ms_per_step"] > 0
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"last_step_request_index.npy", "last_step_new_token_ids.npy",
            "last_step_output_token_ids.npy", "last_step_finished.npy",
            "last_logits_request_index.npy",
            "last_logits_sample.npy"} == set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.shape == y.shape and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    idx = np.load(a / "last_step_request_index.npy")
    new = np.load(a / "last_step_new_token_ids.npy")
    assert len(idx) > 0 and new.shape[0] == len(idx)
    assert (new[:, 0] >= 0).all()
    logits = np.load(a / "last_logits_sample.npy")
    assert logits.shape[0] == len(np.load(a / "last_logits_request_index.npy"))
    assert np.isfinite(logits).all()
