"""bench.py's driver contract on a host without a GPU (--device cpu: the fp32
PyTorch trainer over gloo -- a plumbing check, never a headline number)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_self_spawns_ranks_and_reports_process_group():
    r = _bench(["--device", "cpu", "--gpus", "2", "--model", "cifar_resnet20", "--batch", "8",
                "--steps", "2", "--warmup", "1"], {"DTR_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["pg_world_size"] == 2 and out["dist_backend"] == "gloo"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert out["config"]["global_batch"] == 8 and out["config"]["per_gpu_batch"] == 4
    assert out["config"]["parallelism"] == "dp2" and out["dtype"] == "fp32"
    assert out["config"]["env"].get("DTR_DIST_BACKEND") == "gloo"
    for key in ("metric", "unit", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "data", "config"):
        assert key in out


def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 / float64 .npy, and
    two runs with the same arguments start from the same inputs: identical files."""
    import numpy as np

    dumps = []
    for d in ("a", "b"):
        r = _bench(["--device", "cpu", "--gpus", "1", "--model", "cifar_resnet20", "--batch", "4",
                    "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["bn_moving_stats.npy", "metrics.npy", "metrics_names.txt",
                         "momentum.npy", "weights.npy"]
        dumps.append({f: np.load(tmp_path / d / f) for f in files if f.endswith(".npy")})
    a, b = dumps
    names = (tmp_path / "a" / "metrics_names.txt").read_text().split()
    assert a["metrics.npy"].dtype == np.float64 and len(names) == a["metrics.npy"].size
    assert a["metrics.npy"][names.index("global_step")] == 3      # warmup + steps
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f
    assert a["weights.npy"].ndim == 1 and np.abs(a["momentum.npy"]).sum() > 0


def test_bench_spawn_fails_when_a_rank_fails():
    # an indivisible global batch makes every rank exit non-zero
    r = _bench(["--device", "cpu", "--gpus", "2", "--model", "cifar_resnet20", "--batch", "7",
                "--steps", "1", "--warmup", "0"], {"DTR_DIST_BACKEND": "gloo"})
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_refuses_diagnostic_and_unsupported_modes():
    r = _bench(["--device", "cpu", "--steps", "1"], {"DTR_DIAG_SKIP": "wgrad"})
    assert r.returncode == 2 and "DTR_DIAG_SKIP" in r.stderr
    r = _bench(["--gpus", "2", "--graph"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "--graph" in r.stderr
    r = _bench(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2
