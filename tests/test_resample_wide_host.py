"""The wide (int32 Q31) form of the rate converter on the host (tfp_resample_wide_pcm) against its definition
restated in Python big integers over the pair's own table (tfp_resample_taps), the widening identity that pins
it to the int16 forms, the extremes, short inputs, the range bound A C < 2^30, and the float-to-Q31 maps
(tfp_q31_from_f32 / tfp_q31_from_f64). No GPU.

The absolute tap sums A = max_p sum_k |h[p][k]| that test_abs_sum_bound prints (this Kaiser sinc, Z = 24,
beta = 8), as recorded when the test was written: 16000 -> 8000: 66,592; 44100 -> 8000: 66,258;
8000 -> 16000: 70,208; 7999 -> 8001: 70,210; 96000 -> 8000: 66,196; 192000 -> 8000: 66,144; 1 -> 1000: 70,208.
The largest seen is 70,210 (7999 -> 8001), about 2.14 * 32768, so A * 32 stays below 2^22, far under the 2^30
a wide call needs. (The taps come from libm's sin in double, so another libm may move a figure by a unit.)"""
import ctypes as C

import numpy as np
import pytest

from resample_util import noise
from resample_wide_util import INT32_MAX, INT32_MIN, abs_sum, wide_convolve, wide_mean, wide_noise, wide_reference

PAIRS = [(16000, 8000), (44100, 8000), (8000, 16000), (8000, 8000)]
CHANNELS = [1, 2, 3, 32]
TFP_E_ARG, TFP_E_CAPACITY = -1, -5


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_equals_the_restatement_and_the_int16_forms(tfp_lib, pair, ch):
    t = tfp_lib.resample_taps(*pair)
    n = 3 * t["ntaps"] + 41 if pair[0] != pair[1] else 700
    q = wide_noise(n, ch, 100 * ch + pair[0] % 97)
    got = tfp_lib.resample_wide_pcm(q, ch, *pair)
    assert got.dtype == np.int16 and np.array_equal(got, wide_reference(q, t, *pair))
    # the widening identity: int16 frames x as x << 16 are the mix form of x, and for one channel the rate form
    x = noise(n * ch, 7 + ch).reshape(n, ch)
    wide = tfp_lib.resample_wide_pcm(x.astype(np.int32) << 16, ch, *pair)
    assert np.array_equal(wide, tfp_lib.resample_mix_pcm(x, ch, *pair))
    if ch == 1:
        assert np.array_equal(wide, tfp_lib.resample_pcm(x.reshape(-1), *pair))
    # 24-bit values << 8
    q24 = (np.random.default_rng(ch).integers(-2**23, 2**23, (n, ch)).astype(np.int32)) << 8
    assert np.array_equal(tfp_lib.resample_wide_pcm(q24, ch, *pair), wide_reference(q24, t, *pair))


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_extremes_clamp_without_overflow(tfp_lib, pair):
    t = tfp_lib.resample_taps(*pair)
    n = 2 * t["ntaps"] + 9
    for ch in (1, 32):
        for v, rail in ((INT32_MIN, -32768), (INT32_MAX, 32767)):
            q = np.full((n, ch), v, np.int32)
            got = tfp_lib.resample_wide_pcm(q, ch, *pair)
            assert np.array_equal(got, wide_reference(q, t, *pair))
            mid = got[len(got) // 2]  # away from the clip's ends a constant stays that constant
            assert mid == rail and got.min() >= -32768 and got.max() <= 32767
    # Q31 full scale at equal rates rounds to 32768: the clamp
    assert tfp_lib.resample_wide_pcm(np.array([[INT32_MAX]], np.int32), 1, 8000, 8000)[0] == 32767
    assert wide_mean(np.array([[INT32_MAX]], np.int32))[0] == 32767 and (INT32_MAX + 2**15) // 2**16 == 32768


@pytest.mark.parametrize("ch", [1, 2, 32])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_short_inputs(tfp_lib, pair, ch):
    t = tfp_lib.resample_taps(*pair)
    for n in (0, 1, 2, t["ntaps"] // 2, t["ntaps"] - 1):
        q = wide_noise(n, ch, n + ch)
        got = tfp_lib.resample_wide_pcm(q, ch, *pair)
        want_len = n if pair[0] == pair[1] else max(tfp_lib.resample_count(n, *pair), 0)
        assert len(got) == want_len and np.array_equal(got, wide_reference(q, t, *pair))


def test_abs_sum_bound(tfp_lib):
    """A for the pairs the tests use and for four more at the table's edges; A * 32 < 2^30 for every one."""
    seen = {}
    for pair in [(16000, 8000), (44100, 8000), (8000, 16000), (7999, 8001), (96000, 8000), (192000, 8000), (1, 1000)]:
        a = abs_sum(tfp_lib.resample_taps(*pair))
        seen[pair] = a
        print("A(%d -> %d) = %d" % (pair + (a,)))
        assert a * 32 < 2**30, (pair, a)
        assert a >= 32768  # every phase sums to 32768
    assert max(seen.values()) * 32 < 2**22, seen  # what the header and the README say of the pairs met so far


def test_size_query_capacity_and_refusals(tfp_lib):
    lib = tfp_lib.lib()
    q = wide_noise(1000, 2, 1).reshape(-1)
    n = C.c_int64(-7)
    assert lib.tfp_resample_wide_pcm(q.ctypes.data, 1000, 2, 44100, 8000, None, 0, C.byref(n)) == 0
    assert n.value == tfp_lib.resample_count(1000, 44100, 8000)
    out = np.full(n.value, 77, np.int16)
    m = C.c_int64(-7)
    assert lib.tfp_resample_wide_pcm(q.ctypes.data, 1000, 2, 44100, 8000, out.ctypes.data, n.value - 1, C.byref(m)) == TFP_E_CAPACITY
    assert m.value == n.value and (out == 77).all()
    assert lib.tfp_resample_wide_pcm(q.ctypes.data, 1000, 2, 8000, 8000, None, 0, C.byref(m)) == 0 and m.value == 1000
    for ch, rin, rout, msg in ((0, 44100, 8000, "unsupported channel count"), (33, 44100, 8000, "unsupported channel count"),
                               (2, 0, 8000, "bad sample rate"), (2, 8000, -1, "bad sample rate"),
                               (2, 7999, 44100, "unsupported rate ratio")):
        m = C.c_int64(-7)
        assert lib.tfp_resample_wide_pcm(q.ctypes.data, 1000, ch, rin, rout, out.ctypes.data, len(out), C.byref(m)) == TFP_E_ARG
        assert msg in lib.tfp_engine_last_error(None).decode() and m.value == -7 and (out == 77).all()
    assert lib.tfp_resample_wide_pcm(None, 5, 2, 44100, 8000, None, 0, C.byref(m)) == TFP_E_ARG
    assert lib.tfp_resample_wide_pcm(q.ctypes.data, -1, 2, 44100, 8000, None, 0, C.byref(m)) == TFP_E_ARG


def test_q31_from_f32(tfp_lib):
    f = np.float32
    tiny32 = np.finfo(np.float32).smallest_subnormal
    cases = [(1.0, INT32_MAX), (-1.0, INT32_MIN), (f(1) - f(2.0**-24), 2**31 - 128), (-(f(1) - f(2.0**-24)), -(2**31 - 128)),
             (2.0**-9, 2**22), (2.0**-31, 1), (2.0**-32, 0), (3 * 2.0**-32, 2), (5 * 2.0**-32, 2), (-(2.0**-32), 0),
             (-3 * 2.0**-32, -2), (2.0**-33, 0), (0.75 * 2.0**-31, 1), (tiny32, 0), (-tiny32, 0), (2.0**-126, 0), (0.0, 0),
             (-0.0, 0), (np.nan, 0), (np.inf, INT32_MAX), (-np.inf, INT32_MIN), (2.0, INT32_MAX), (-2.0, INT32_MIN),
             (0.5, 2**30), (-0.5, -2**30), (1e38, INT32_MAX)]
    x = np.array([c[0] for c in cases], np.float32)
    got = tfp_lib.q31_from_float(x)
    assert got.dtype == np.int32 and got.tolist() == [c[1] for c in cases]
    # against the exact value: x 2^31 is exact in Python's double for every float32, round() ties to even
    r = np.random.default_rng(3).standard_normal(4096).astype(np.float32) * f(0.5)
    want = [min(max(round(float(v) * 2.0**31), INT32_MIN), INT32_MAX) for v in r]
    assert tfp_lib.q31_from_float(r).tolist() == want


def test_q31_from_f64(tfp_lib):
    tiny = np.finfo(np.float64).smallest_subnormal
    cases = [(1.0, INT32_MAX), (-1.0, INT32_MIN), (1 - 2.0**-24, 2**31 - 128), (1 - 2.0**-32, INT32_MAX), (1 - 2.0**-31, INT32_MAX),
             (1 - 3 * 2.0**-32, 2**31 - 2), (2.0**-9, 2**22), (2.0**-31, 1), (2.0**-32, 0), (3 * 2.0**-32, 2), (5 * 2.0**-32, 2),
             (7 * 2.0**-32, 4), (-(2.0**-32), 0), (-3 * 2.0**-32, -2), (-5 * 2.0**-32, -2), (2.0**-32 + 2.0**-60, 1), (tiny, 0),
             (-tiny, 0), (2.0**-1022, 0), (0.0, 0), (-0.0, 0), (np.nan, 0), (np.inf, INT32_MAX), (-np.inf, INT32_MIN),
             (-1 - 2.0**-32, INT32_MIN), (1e300, INT32_MAX), (-1e300, INT32_MIN)]
    x = np.array([c[0] for c in cases], np.float64)
    got = tfp_lib.q31_from_float(x)
    assert got.tolist() == [c[1] for c in cases]
    r = np.random.default_rng(4).standard_normal(4096) * 0.5
    want = [min(max(round(float(v) * 2.0**31), INT32_MIN), INT32_MAX) for v in r]
    assert tfp_lib.q31_from_float(r).tolist() == want
    lib = tfp_lib.lib()
    assert lib.tfp_q31_from_f64(None, 3, None) == TFP_E_ARG and lib.tfp_q31_from_f32(None, -1, None) == TFP_E_ARG
    assert lib.tfp_q31_from_f32(None, 0, None) == 0
