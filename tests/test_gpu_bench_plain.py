"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` run -- set up, warm up, K timed steps, the line -- and --dump-outputs.  More
steps than one walk of the drives holds (LAP_FRAMES frames per drive) walk them again: the line still counts K steps, and the last step of
the second walk registers the same pair from the same history as the last step of a run that ends inside the first walk."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--detail-out", str(tmp_path / "detail.json")],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(rows) == 1 and out.stdout.strip().splitlines()[-1] == rows[0]
    return json.loads(rows[0])


@pytest.mark.timeout(900)
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    import bench
    lap = bench.LAP_FRAMES - 2 - 2                           # timed steps per walk at --warmup 2
    long_steps = lap + 7
    line = _run(["--steps", str(long_steps), "--warmup", "2", "--dump-outputs", str(tmp_path / "long")], tmp_path)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in line, key
    for key in ("configs", "cpu_baseline", "host_inputs", "timed_pairs_vs_oracle", "single_pair", "against_simulated_motion"):
        assert key not in line, key                          # --full only
    assert line["steps"] == long_steps and line["warmup"] == 2 and line["unit"] == "scan-pairs/s"
    assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) < 1e-4 * line["value"]
    assert line["config"]["frames_per_drive"] == bench.LAP_FRAMES and line["config"]["distinct_pairs"] == lap * 8
    assert line["chain"]["calls"] == long_steps * 8
    short = _run(["--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "short")], tmp_path)
    assert short["steps"] == 7 and short["config"]["frames_per_drive"] == 7 + 2 + 2
    names = sorted(os.listdir(tmp_path / "long"))
    assert names == sorted(os.listdir(tmp_path / "short")) == ["next_guess.npy", "pose_T.npy", "pose_x.npy", "solve_stats.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "long" / n), np.load(tmp_path / "short" / n)
        total += a.nbytes
        assert a.dtype == np.float64 and a.shape == b.shape and a.shape[0] == 8, n
        assert np.all(np.isfinite(a)) or n == "solve_stats.npy", n
        assert np.allclose(a, b, rtol=1e-9, atol=1e-9, equal_nan=True), (n, np.nanmax(np.abs(a - b)))
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "long" / "pose_x.npy")[0], np.array(line["solution_x"]))


@pytest.mark.timeout(900)
def test_full_run_whose_steps_end_inside_a_walk(tmp_path):
    """--full behind timed steps that end inside the second walk of the drives: the drives are walked to their last frame off the clock
    before the single-pair walk restarts a context, and the oracle replays timed pairs of the first walk"""
    import bench
    lap = bench.LAP_FRAMES - 2 - 2
    line = _run(["--steps", str(lap + 7), "--warmup", "2", "--full", "--no-legs", "--no-cpu-baseline"], tmp_path)
    assert line["steps"] == lap + 7 and line["chain"]["calls"] == (lap + 7) * 8
    tp = line["timed_pairs_vs_oracle"]
    assert tp["ok"] is True and tp["counts_equal"] is True and tp["pairs"] == 2
    assert line["single_pair"]["pairs_per_s"] > 0 and line["against_simulated_motion"]["pairs"] == (lap + 7) * 8
