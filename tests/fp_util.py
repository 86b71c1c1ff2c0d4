"""Shared by the fingerprint tests: the bit-exact frame comparison against the CPU oracle, and the
launch counter's bookkeeping (Engine.fingerprint_stats: which fingerprint kernel a call ran)."""
import numpy as np

KERNELS = ("small8k", "throughput8k", "generic_i16", "generic_f32")


def assert_frames_equal(fr, micro, db):
    assert len(fr) == len(micro)
    bad = (fr["m1"] != micro[:, 0]) | (fr["m2"] != micro[:, 1])
    if bad.any():
        i = np.nonzero(bad)[0]
        print("mismatching frames:", len(i), "of", len(fr), "first:", i[:10])
        print("gpu q1,q2:", fr["q1"][i[:5]], fr["q2"][i[:5]])
        print("cpu q1,q2:", db[i[:5], 0], db[i[:5], 1])
    assert np.array_equal(fr["m1"], micro[:, 0]), np.nonzero(fr["m1"] != micro[:, 0])
    assert np.array_equal(fr["m2"], micro[:, 1]), np.nonzero(fr["m2"] != micro[:, 1])
    # q: the frame values are glibc's 10*log10|c| bit for bit (tfp_math.hpp LogFix); a NaN is a
    # NaN whatever its payload (x86 and gfx950 make different default NaNs)
    for k, col in (("q1", 0), ("q2", 1)):
        a, b = fr[k], db[:, col]
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), np.nonzero(~same)


def launches_since(eng, before):
    """The fingerprint launches per kernel since `before` (an earlier eng.fingerprint_stats())."""
    now = eng.fingerprint_stats()
    assert tuple(now) == KERNELS
    return {k: now[k] - before[k] for k in KERNELS}


def assert_only_kernel(eng, before, kernel, hint=""):
    """Every fingerprint launch since `before` was `kernel`, and there was at least one."""
    d = launches_since(eng, before)
    assert d[kernel] >= 1 and all(d[k] == 0 for k in KERNELS if k != kernel), (kernel, d, hint)
