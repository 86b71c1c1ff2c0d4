"""bench.py as later measurements run it: a plain run times the fingerprint steps and nothing else,
--steps sets the number of timed steps, and --dump-outputs writes what the last timed step stored
(checked against the CPU oracle on the same synthetic clips). One small run: 5 x 3 s clips."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402

FULL_LEGS = ("strong", "cpu_baseline", "match", "stream", "group")


@pytest.mark.gpu
def test_plain_run_times_steps_only_and_dumps_oracle_values(engine, oracle, tfp_lib, tmp_path):
    clips, seconds, steps = 5, 3, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--clips", str(clips), "--seconds", str(seconds), "--clock-warmup-s", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    got = json.loads(lines[0])
    assert not set(FULL_LEGS) & set(got) and got["full"] is False
    n = 8000 * seconds
    frames = clips * ((n + bench.HOP - 1) // bench.HOP)
    assert got["steps"] == steps and got["unit"] == "fingerprints/s" and got["higher_is_better"] is True
    assert got["dtype"] == "f32" and got["config"]["frames_per_step_per_gpu"] == frames
    assert got["ms_per_step"] > 0 and got["value"] == pytest.approx(frames / (got["ms_per_step"] / 1e3), rel=1e-9)
    assert os.listdir(out) == ["fingerprints.npy"]
    dumped = np.load(out / "fingerprints.npy")
    pcm = tfp_lib.synth_pcm(bench.SEED_DB, range(clips), n)
    micro, _ = oracle.fingerprint_batch(pcm.reshape(-1), np.arange(clips + 1) * n, nthreads=4, want_db=False)
    assert dumped.dtype == np.float64 and dumped.shape == (frames, 2)
    assert np.array_equal(dumped, micro.astype(np.float64))
