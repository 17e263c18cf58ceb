"""bench.py driver-contract regression guard: one JSON line with every
required field (the round driver depends on this exact shape)."""

import json
import os
import subprocess
import sys

import pytest

from tests.conftest import free_port

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


@pytest.mark.timeout(400)
def test_bench_json_contract():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=380, cwd=REPO_ROOT,
        env={**os.environ, "TRACEML_AGGREGATOR_PORT": str(free_port())},
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    json_lines = [
        l for l in proc.stdout.strip().splitlines() if l.startswith("{")
    ]
    assert len(json_lines) == 1, proc.stdout[-1000:]  # exactly ONE JSON line
    payload = json.loads(json_lines[-1])
    assert REQUIRED_KEYS <= set(payload), REQUIRED_KEYS - set(payload)
    assert payload["metric"] == "instrumentation overhead (% step time)"
    assert payload["higher_is_better"] is False
    assert payload["scaling"] == "weak"
    assert payload["n_gpus"] == 1
    assert payload["steps"] == 2 and payload["warmup"] == 1
    assert payload["data"] == "synthetic"
    assert payload["vs_baseline"] is None  # reference publishes no numbers
    config = payload["config"]
    for key in ("model", "global_batch", "parallelism"):
        assert key in config
    assert isinstance(payload["value"], float)
    assert isinstance(payload["ms_per_step"], float)


def _run_bench(*extra):
    proc = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "4",
         "--warmup", "1", "--model", "mlp", *extra],
        capture_output=True, text=True, timeout=380, cwd=REPO_ROOT,
        env=dict(os.environ),
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    json_lines = [
        l for l in proc.stdout.strip().splitlines() if l.startswith("{")
    ]
    assert len(json_lines) == 1, proc.stdout[-1000:]
    return json.loads(json_lines[-1])


@pytest.mark.timeout(400)
def test_bench_plain_run_times_exactly_k_steps():
    """A plain run is lean: the K timed steps are split between the two
    arms, and nothing of the --full protocol runs."""
    payload = _run_bench()
    config = payload["config"]
    assert config["protocol"] == "plain"
    assert config["timed_steps_traced"] + config["timed_steps_untraced"] == 4
    assert "rounds_per_arm" not in config
    assert config["diagnosis"] is None
    assert payload["ms_per_step"] > 0.0
    assert config["ms_per_step_untraced"] > 0.0


@pytest.mark.timeout(400)
def test_bench_full_protocol():
    """--full keeps the rigorous protocol: interleaved rounds of K timed
    steps per arm, the same-arm noise floor and the diagnosis read-back."""
    payload = _run_bench("--full")
    assert REQUIRED_KEYS <= set(payload), REQUIRED_KEYS - set(payload)
    assert payload["metric"] == "instrumentation overhead (% step time)"
    assert payload["steps"] == 4 and payload["warmup"] == 1
    config = payload["config"]
    assert config["protocol"] == "full"
    assert config["rounds_per_arm"] >= 3
    assert isinstance(config["noise_pct_same_arm_spread"], float)
    assert isinstance(config["diagnosis"], str)
    assert isinstance(payload["value"], float)
    assert isinstance(payload["ms_per_step"], float)


@pytest.mark.timeout(400)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy,
    within the size budget, and identically from run to run."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        _run_bench("--dump-outputs", str(out))
        files = sorted(p.name for p in out.iterdir())
        assert files == ["loss.npy", "params.npy"]
        arrays = {f: np.load(out / f) for f in files}
        for arr in arrays.values():
            assert arr.dtype in (np.float32, np.float64)
            assert arr.size > 0 and np.isfinite(arr).all()
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 1024 * 1024
        dumps.append(arrays)
    # same seed, same inputs, same five fp32 steps: only the reduction order
    # inside a GEMM may differ between two runs, a few ulp (2**-23) per value
    for f, arr in dumps[0].items():
        np.testing.assert_allclose(arr, dumps[1][f], rtol=1e-5, atol=1e-6)


@pytest.mark.timeout(500)
def test_bench_gpus8_gloo_exits_clean():
    """The driver's 8-GPU SCALE run, rehearsed on CPU/gloo: bench.py under
    torch.distributed.run ws=8 must negotiate one aggregator port, settle
    all 8 ranks and print exactly one JSON line."""
    proc = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node=8", "--master-addr=127.0.0.1",
            f"--master-port={free_port()}",
            "bench.py", "--gpus", "8", "--steps", "2", "--warmup", "1",
            "--model", "mlp",
        ],
        capture_output=True, text=True, timeout=480, cwd=REPO_ROOT,
        # a CPU/gloo rehearsal wherever it runs: on a machine with fewer
        # than 8 GPUs the 8 ranks could not each take a device
        env={**os.environ, "MASTER_ADDR": "127.0.0.1",
             "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""},
    )
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-3000:])
    json_lines = [
        l for l in proc.stdout.strip().splitlines() if l.startswith("{")
    ]
    assert len(json_lines) == 1, proc.stdout[-1500:]
    payload = json.loads(json_lines[-1])
    assert payload["n_gpus"] == 8
    assert payload["config"]["parallelism"] == "dp8"
    assert payload["config"]["global_batch"] == 32 * 8


@pytest.mark.timeout(400)
def test_bench_llama3_and_gpt2_arms_runnable():
    """BASELINE configs 4/5 are driver-runnable arms: each prints the JSON
    contract line with its integration path recorded."""
    for model, path_word in (("llama3", "HF"), ("gpt2", "Lightning")):
        proc = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--model", model],
            capture_output=True, text=True, timeout=180, cwd=REPO_ROOT,
            env=dict(os.environ),
        )
        assert proc.returncode == 0, (model, proc.stderr[-2000:])
        json_lines = [
            l for l in proc.stdout.strip().splitlines() if l.startswith("{")
        ]
        assert len(json_lines) == 1, (model, proc.stdout[-1000:])
        payload = json.loads(json_lines[-1])
        assert payload["config"]["model"] == model
        assert path_word in payload["config"]["integration_path"]
        assert payload["config"]["self_overhead_us_per_step"] is not None
