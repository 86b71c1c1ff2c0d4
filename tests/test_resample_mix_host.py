"""The host side of multichannel rate-normalised ingest (tfp_resample_mix_pcm): one channel against
tfp_resample_pcm, several against an int64 numpy restatement, the floor and the tie in closed form, full scale
through the 64-bit product and the clamp, the integer mean at equal rates, and the refusals. No GPU."""
import ctypes as C

import numpy as np
import pytest

from resample_mix_util import mix_convolve, mix_mean, mix_noise
from resample_util import PAIRS, TILE, edge_lengths, noise, plan, rails

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
HOST_PAIRS = [(16000, 8000), (8000, 16000), (44100, 8000), (11025, 8000)]


def _last_error(tfp_lib):
    return (tfp_lib.lib().tfp_engine_last_error(None) or b"").decode()


@pytest.mark.parametrize("pair", list(PAIRS), ids=lambda p: "%d-%d" % p)
def test_one_channel_is_resample_pcm(tfp_lib, pair):
    t = tfp_lib.resample_taps(*pair)
    lens = [4001] + (edge_lengths(t, TILE) if t["taps"].size < 100000 else edge_lengths(t, TILE)[:5])
    for n in lens:
        x = noise(n, 300 + n)
        assert np.array_equal(tfp_lib.resample_mix_pcm(x, 1, *pair), tfp_lib.resample_pcm(x, *pair)), (pair, n)


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("ch", [2, 3, 6])
def test_routine_equals_the_restatement(tfp_lib, pair, ch):
    t = tfp_lib.resample_taps(*pair)
    for n in (0, 1, 2, t["ntaps"] - 1, t["ntaps"], 4001):
        x = mix_noise(n, ch, 100 + n + ch)
        y = tfp_lib.resample_mix_pcm(x, ch, *pair)
        assert y.dtype == np.int16 and len(y) == tfp_lib.resample_count(n, *pair)
        assert np.array_equal(y, mix_convolve(x, t)), (pair, ch, n)


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
def test_closed_form_pins_the_floor_and_the_tie(tfp_lib, pair):
    """Every frame's channel sum is S: each phase sums to 32768, so an output whose filter lies wholly inside
    the clip is floor((2 S + C) / (2 C)). S = -5, C = 3 gives -2 (truncation: -1); S = -3, C = 2 gives -1."""
    L, M, k_lo, k_hi = plan(*pair)
    edge = max(k_hi * M // L + 1, -(-(k_hi * L) // M) + 1)
    for ch in (2, 3):
        for S in (-5, -4, -3, -1, 1, 3, 4, 5):
            x = np.zeros((20000, ch), np.int16)
            x[:, 0] = S  # channel 0 carries the sum
            if ch == 3:
                x[:, 1], x[:, 2] = 7, -7
            y = tfp_lib.resample_mix_pcm(x, ch, *pair)
            assert len(y) > 2 * edge + 100
            want = (2 * S + ch) // (2 * ch)
            assert (y[edge + 1:len(y) - edge - 1] == want).all(), (pair, ch, S, want)
    assert (2 * -5 + 3) // 6 == -2 and (2 * -3 + 2) // 4 == -1


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("ch", [3, 32])
def test_full_scale(tfp_lib, pair, ch):
    t = tfp_lib.resample_taps(*pair)
    for v in (-32768, 32767):
        x = np.full((3000, ch), v, np.int16)
        y = tfp_lib.resample_mix_pcm(x, ch, *pair)
        assert np.array_equal(y, mix_convolve(x, t)), (pair, ch, v)
        assert (y == v).any()
    r = rails(6000, max(t["M"], 8))
    x = np.repeat(r[:, None], ch, axis=1)
    y = tfp_lib.resample_mix_pcm(x, ch, *pair)
    assert (y == 32767).any() and (y == -32768).any()  # the clamp is exercised, both ways
    assert np.array_equal(y, mix_convolve(x, t))
    assert np.array_equal(y, tfp_lib.resample_pcm(r, *pair))  # equal channels: the mono conversion of one of them


def test_equal_rates_are_the_integer_mean(tfp_lib):
    for ch in (2, 3, 6, 32):
        x = mix_noise(4001, ch, 9 + ch)
        for r in (8000, 44100, 1):
            y = tfp_lib.resample_mix_pcm(x, ch, r, r)
            assert len(y) == 4001 and np.array_equal(y, mix_mean(x))
    x = np.array([[-3, 0], [-1, 0], [1, 0], [32767, 32767], [-32768, -32768], [-5, 2]], np.int16)
    assert tfp_lib.resample_mix_pcm(x, 2, 8000, 8000).tolist() == [-1, 0, 1, 32767, -32768, -1]
    assert len(tfp_lib.resample_mix_pcm(np.zeros((0, 2), np.int16), 2, 8000, 8000)) == 0


def test_refusals_and_capacity(tfp_lib):
    lib = tfp_lib.lib()
    x = mix_noise(1000, 2, 5)
    out = np.full(400, 77, np.int16)
    for ch in (0, 33, -1):
        n = C.c_int64(-7)
        assert lib.tfp_resample_mix_pcm(x.ctypes.data, 10, ch, 44100, 8000, out.ctypes.data, 400, C.byref(n)) == TFP_E_ARG
        assert "unsupported channel count" in _last_error(tfp_lib) and n.value == -7 and (out == 77).all()
    for a, b in ((0, 8000), (8000, 0), (-1, 8000), (8000, -1)):
        n = C.c_int64(-7)
        assert lib.tfp_resample_mix_pcm(x.ctypes.data, 1000, 2, a, b, out.ctypes.data, 400, C.byref(n)) == TFP_E_ARG
        assert "bad sample rate" in _last_error(tfp_lib) and n.value == -7 and (out == 77).all()
    n = C.c_int64(-7)
    assert lib.tfp_resample_mix_pcm(x.ctypes.data, 1000, 2, 7999, 44100, out.ctypes.data, 400, C.byref(n)) == TFP_E_ARG
    assert "unsupported rate ratio" in _last_error(tfp_lib) and n.value == -7 and (out == 77).all()
    n = C.c_int64()
    assert lib.tfp_resample_mix_pcm(x.ctypes.data, 1000, 2, 44100, 8000, None, 0, C.byref(n)) == 0  # size query
    need = n.value
    assert need == tfp_lib.resample_count(1000, 44100, 8000) == 182
    n = C.c_int64()
    assert lib.tfp_resample_mix_pcm(x.ctypes.data, 1000, 2, 44100, 8000, out.ctypes.data, need - 1, C.byref(n)) == TFP_E_CAPACITY
    assert n.value == need and (out == 77).all()
    assert lib.tfp_resample_mix_pcm(x.ctypes.data, 1000, 2, 44100, 8000, out.ctypes.data, need, C.byref(n)) == 0
    assert np.array_equal(out[:need], mix_convolve(x, tfp_lib.resample_taps(44100, 8000))) and (out[need:] == 77).all()
