"""The throughput launch without doubles (tfp_fingerprint_device with d_db = NULL): one kernel whose tile
tail finishes the micro-units with the fast exact finish (csrc/tfp_math.hpp micro_of_coef_fast).

A batch of just over 256 16-frame tiles (the smallest that takes the throughput kernel, asserted with
the launch counter) whose clips sit at the tail's edges: 1, 255, 256 and 257 samples, exactly 16 frames,
16 frames plus a sample, 10 frames past a tile boundary (a tile whose last passes are empty), clips
on odd samples (every clip after an odd-length one) and all-zero clips. The
micro-units equal the oracle's bit for bit, equal the same call with d_db given (raw float bits, then
finish_db_kernel), and are the same on an engine whose margin knob sends every value through the
tail's slow branch. The helper itself is checked on the GPU over the host test's sampled patterns
(tests/native/check_micro_fast.hip)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from fp_util import assert_only_kernel
from test_gpu_parity import _engine_with

pytestmark = pytest.mark.gpu

LENGTHS = [1, 255, 256, 257, 16 * 256, 16 * 256 + 1, 26 * 256, 777, 3000]
ROUNDS = 24  # 216 clips, 11 tiles per round


class Batch:
    pass


@pytest.fixture(scope="module")
def batch(oracle, tfp_lib):
    rng = np.random.default_rng(0xF1)
    lens = np.array(LENGTHS * ROUNDS, np.int64)
    clips = []
    for i, n in enumerate(lens):
        kind = i % 4
        if kind == 0:
            c = rng.integers(-32768, 32768, n).astype(np.int16)
        elif kind == 1:
            c = tfp_lib.synth_pcm(0x7153A1, [i], int(n))[0]
        elif kind == 2:
            c = rng.integers(-3, 4, n).astype(np.int16)
        else:
            c = np.zeros(n, np.int16)  # every band at the log's clamp: one constant row
        clips.append(c)
    b = Batch()
    b.flat = np.concatenate(clips)
    b.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nfr = (lens + 255) // 256
    b.nframes = int(nfr.sum())
    assert 256 < int(((nfr + 15) // 16).sum()) <= 300
    start = b.off[:-1]
    for n in LENGTHS:  # every length starts on an odd sample somewhere, and is all-zero somewhere
        assert any(int(s) % 2 == 1 for s, m in zip(start, lens) if m == n)
        assert any(i % 4 == 3 for i, m in enumerate(lens) if m == n)
    b.micro, _ = oracle.fingerprint_batch(b.flat, b.off, nthreads=8, want_db=False)
    assert len(b.micro) == b.nframes
    return b


def _device_micro(eng, b, with_db):
    torch = pytest.importorskip("torch")
    pcm = torch.from_numpy(b.flat).cuda()
    plan = eng.plan(b.off)
    assert plan.nframes == b.nframes
    micro = torch.full((plan.nframes, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    db = torch.zeros((plan.nframes, 2), dtype=torch.float64, device="cuda") if with_db else None
    st = eng.fingerprint_stats()
    eng.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), db.data_ptr() if with_db else 0,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_only_kernel(eng, st, "throughput8k", "the batch is a small one now: raise ROUNDS")
    return micro.cpu().numpy()


def test_fused_finish_equals_oracle_and_split_path(engine, batch):
    fused = _device_micro(engine, batch, with_db=False)
    assert np.array_equal(fused, batch.micro), np.nonzero(fused != batch.micro)
    split = _device_micro(engine, batch, with_db=True)
    assert np.array_equal(split, fused), np.nonzero(split != fused)


def test_fused_finish_slow_branch(batch, tfp_lib):
    """Margin 2^0 micro-units: no value is decided, every tile takes the in-kernel slow branch."""
    eng = _engine_with(tfp_lib, {"TFP_FINISH_MARGIN_LOG2": "0"})
    try:
        slow = _device_micro(eng, batch, with_db=False)
    finally:
        eng.close()
    assert np.array_equal(slow, batch.micro), np.nonzero(slow != batch.micro)


def test_micro_fast_on_gpu():
    exe = os.path.join(PKG, "bin", "check_micro_fast")
    assert os.path.exists(exe), "build with make -C asterisk-tiresias_amd"
    r = subprocess.run([exe, "997", os.path.join(REPO, "tests", "golden", "micro_fast_boundary.txt")],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "gpu != host on 0, gpu != glibc on 0" in r.stdout
