"""bench.py's plain run, --dump-outputs and --full.

A plain run times --steps passes and prints the headline line only; the side
legs (roofline, tracking, DARE, per-step API, CPU baseline) appear with --full.
--dump-outputs writes the last timed pass's arrays, which are the fused
rollout's results for the same seeded episodes bit for bit."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SIDE_LEGS = ("roofline", "cpu_baseline", "tracking", "dare", "step_api")
N = 4160  # 65 waves: not a multiple of the 256-episode block


def _run(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--episodes", str(N), "--warmup", "1",
                        "--warmup-seconds", "0", *argv], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    line = _run("--steps", "3", "--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in line
    assert not [k for k in SIDE_LEGS if k in line]
    assert line["steps"] == 3 and line["unit"] == "env-steps/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    met = np.load(tmp_path / "metrics.npy")
    # value = executed env-steps of a pass x steps / the timed seconds
    env_steps = float(met[-1].sum())
    assert line["value"] == pytest.approx(env_steps / (line["ms_per_step"] * 1e-3), rel=1e-3)

    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop

    ref = run_closed_loop(BatchedRiccatiLQR({"dt": 0.01}, device="cuda:0"), {"target": {"motion_type": "linear"}},
                          n=N, seeds=np.arange(N))
    want = {"metrics": ref.metrics, "state_x": ref.state.x, "state_target": ref.state.target, "state_t": ref.state.t,
            "state_acc": ref.state.acc, "state_integ": ref.state.integ}
    total = 0
    for name, t in want.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64
        assert np.array_equal(got, t.cpu().numpy()), name
        total += got.nbytes
    assert np.array_equal(np.load(tmp_path / "episode_index.npy"), np.arange(N))
    part = np.load(tmp_path / "summary_partials.npy")
    assert part.shape == (11,) and part[4] == N
    assert part[1] == pytest.approx(met[2].sum(), rel=1e-12)  # sum of the mean tracking errors
    assert total < 64e6


@pytest.mark.gpu
def test_full_run_adds_the_side_legs():
    line = _run("--steps", "2", "--full", "--cpu-sample", "256", "--cpu-sample-1core", "64", "--cpu-threads", "2",
                "--step-api-episodes", "4096", "--step-api-steps", "5")
    for k in HEADLINE + SIDE_LEGS:
        assert line.get(k) is not None, k
    # the bound smoke() holds the GPU to against the oracle
    assert line["tracking"]["oracle_sample_max_abs_diff"] < 1e-5
    assert line["step_api"]["check_vs_fused_max_abs_diff"] < 1e-5
    assert line["dare"]["problems"] == N


def test_dump_outputs_samples_within_the_limit(tmp_path, monkeypatch):
    """Arrays beyond the byte limit keep one fixed, sorted sample of episodes,
    the same for every array and every run."""
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 200_000)
    n = 10_000
    a = torch.arange(3 * n, dtype=torch.float64).reshape(3, n)
    b = torch.arange(n, dtype=torch.float64)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, {"a": a, "b": b}, {"s": torch.ones(11, dtype=torch.float64)})
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == ["a.npy", "b.npy", "episode_index.npy", "s.npy"]
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in files) <= 200_000
    idx = np.load(tmp_path / "one" / "episode_index.npy").astype(np.int64)
    assert 1000 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "one" / "b.npy"), idx)
    assert np.array_equal(np.load(tmp_path / "one" / "a.npy"), a.numpy()[:, idx])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))
    # a rank other than 0 of a 2-rank run: half the limit, its own file names
    bench.dump_outputs(str(tmp_path / "r1"), 1, 2, {"a": a}, {})
    assert sorted(os.listdir(tmp_path / "r1")) == ["a.rank1.npy", "episode_index.rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "r1" / f) for f in os.listdir(tmp_path / "r1")) <= 100_000
