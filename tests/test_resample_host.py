"""The host side of rate-normalised ingest (tfp_resample_count / _taps / _pcm): the table against the
formula, the routine against an int64 numpy restatement over the library's own table, the conventions of
the size query, and a derived error bound against the unrounded filter. No GPU. The index arithmetic at
its edges runs stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/native/check_resample.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from resample_util import PAIRS, convolve, count, formula_taps, noise, plan, rails

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
SEVEN = [p for p in PAIRS if p != (8001, 8000)]
HOST_PAIRS = [(16000, 8000), (8000, 16000), (44100, 8000), (11025, 8000)]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def _last_error(tfp_lib):
    return (tfp_lib.lib().tfp_engine_last_error(None) or b"").decode()


@pytest.mark.parametrize("pair", SEVEN, ids=lambda p: "%d-%d" % p)
def test_table_is_the_formula(tfp_lib, pair):
    t = tfp_lib.resample_taps(*pair)
    L, M, k_lo, k_hi = plan(*pair)
    assert (t["L"], t["M"], t["k_lo"], t["ntaps"]) == (L, M, k_lo, k_hi - k_lo + 1)
    assert (L, M, t["ntaps"]) == PAIRS[pair]
    taps = t["taps"].astype(np.int64)
    assert taps.shape == (L, t["ntaps"]) and t["taps"].dtype == np.int16  # every tap fits int16
    assert (taps.sum(axis=1) == 32768).all()
    want = formula_taps(*pair)
    err = np.abs(taps - want)
    # every tap within 1 of the formula, but for the adjusted one: at most one tap per phase, a largest tap
    # of its phase (two taps tie where a phase is symmetric), within ntaps / 2 + 1
    off = err > 1.0
    assert (off.sum(axis=1) <= 1).all()
    assert (err[off] <= t["ntaps"] / 2 + 1).all(), err.max()
    assert (want[off] >= (want.max(axis=1, keepdims=True) - 1.0).repeat(t["ntaps"], axis=1)[off]).all()
    # recomputed, not pinned: the largest tap and the largest sum of magnitudes the accumulator must hold
    print(pair, "max tap", taps.max(), "max sum|h|", np.abs(taps).sum(axis=1).max())
    assert np.abs(taps).sum(axis=1).max() * 32768 < 2**62


def test_limits_and_errors(tfp_lib):
    lib = tfp_lib.lib()
    t = tfp_lib.resample_taps(8001, 8000)
    assert (t["L"], t["M"], t["ntaps"]) == PAIRS[(8001, 8000)] and t["taps"].size == 400000
    assert (t["taps"].astype(np.int64).sum(axis=1) == 32768).all()
    v = [C.c_int32(-7) for _ in range(4)]
    refs = [C.byref(x) for x in v]
    assert lib.tfp_resample_taps(7999, 44100, *refs, None, 0) == TFP_E_ARG
    assert "unsupported rate ratio" in _last_error(tfp_lib)
    assert tfp_lib.resample_count(100, 7999, 44100) == -1
    for bad in (0, -1):
        for a, b in ((bad, 8000), (8000, bad)):
            assert lib.tfp_resample_taps(a, b, *refs, None, 0) == TFP_E_ARG
            assert "bad sample rate" in _last_error(tfp_lib)
            assert tfp_lib.resample_count(100, a, b) == -1
            n = C.c_int64(-7)
            x = np.zeros(4, np.int16)
            assert lib.tfp_resample_pcm(x.ctypes.data, 4, a, b, x.ctypes.data, 4, C.byref(n)) == TFP_E_ARG
            assert n.value == -7 and "bad sample rate" in _last_error(tfp_lib)
    assert [x.value for x in v] == [-7] * 4
    assert tfp_lib.resample_count(0, 16000, 8000) == 0 and tfp_lib.resample_count(-5, 16000, 8000) == 0


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
def test_routine_equals_the_restatement(tfp_lib, pair):
    t = tfp_lib.resample_taps(*pair)
    for n in (0, 1, 2, t["ntaps"] - 1, t["ntaps"], 4001):
        x = noise(n, 100 + n)
        y = tfp_lib.resample_pcm(x, *pair)
        assert y.dtype == np.int16 and len(y) == tfp_lib.resample_count(n, *pair) == count(n, t["L"], t["M"])
        assert np.array_equal(y, convolve(x, t)), (pair, n)


def test_size_query_and_capacity(tfp_lib):
    lib = tfp_lib.lib()
    x = noise(1000, 5)
    n = C.c_int64()
    assert lib.tfp_resample_pcm(x.ctypes.data, 1000, 44100, 8000, None, 0, C.byref(n)) == 0
    need = n.value
    assert need == tfp_lib.resample_count(1000, 44100, 8000) == 182
    out = np.full(need, 77, np.int16)
    n = C.c_int64()
    assert lib.tfp_resample_pcm(x.ctypes.data, 1000, 44100, 8000, out.ctypes.data, need - 1, C.byref(n)) == TFP_E_CAPACITY
    assert n.value == need and (out == 77).all()
    v = [C.c_int32() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    taps = np.full(97, 77, np.int16)
    assert lib.tfp_resample_taps(16000, 8000, *refs, taps.ctypes.data, 96) == TFP_E_CAPACITY
    assert [x.value for x in v] == [1, 2, -48, 97] and (taps == 77).all()
    assert lib.tfp_resample_taps(16000, 8000, *refs, taps.ctypes.data, 97) == 0 and int(taps.astype(np.int64).sum()) == 32768


def test_equal_rates_are_the_identity(tfp_lib):
    x = noise(4001, 9)
    for r in (8000, 44100, 1):
        assert np.array_equal(tfp_lib.resample_pcm(x, r, r), x)
        assert tfp_lib.resample_count(4001, r, r) == 4001
    assert len(tfp_lib.resample_pcm(np.zeros(0, np.int16), 8000, 8000)) == 0


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
def test_constant_stays_constant(tfp_lib, pair):
    L, M, k_lo, k_hi = plan(*pair)
    y = tfp_lib.resample_pcm(np.full(20000, 12345, np.int16), *pair)
    # more than k_hi M / L + 1 outputs from either end; going up in rate (L > M) the filter's k_hi input
    # samples are k_hi L / M outputs, so the margin is the larger of the two
    edge = max(k_hi * M // L + 1, -(-(k_hi * L) // M) + 1)
    assert len(y) > 2 * edge + 100
    assert (y[edge + 1:len(y) - edge - 1] == 12345).all()


@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "%d-%d" % p)
def test_full_scale_alternation_reaches_both_rails(tfp_lib, pair):
    t = tfp_lib.resample_taps(*pair)
    x = rails(6000, max(t["M"], 8))
    y = tfp_lib.resample_pcm(x, *pair)
    assert (y == 32767).any() and (y == -32768).any()  # the clamp is exercised, both ways
    assert np.array_equal(y, convolve(x, t))


@pytest.mark.parametrize("hz", [1000, 3000])
def test_derived_bound_against_the_unrounded_filter(tfp_lib, hz):
    """|y_int - y_double| <= 0.5 + sum_k |h_int - 32768 h_double| for |x| <= 32768: the rounding of the output
    plus the taps' own rounding times full scale (the sums scaled by 2^-15), per phase, from the table."""
    pair = (44100, 8000)
    t = tfp_lib.resample_taps(*pair)
    want = formula_taps(*pair)
    x = np.rint(30000 * np.sin(2 * np.pi * hz * np.arange(8000) / 44100.0)).astype(np.int16)
    y = tfp_lib.resample_pcm(x, *pair).astype(np.float64)
    yd = convolve(x, t, taps=want)
    bound = 0.5 + np.abs(t["taps"].astype(np.float64) - want).sum(axis=1)
    ph = (np.arange(len(y), dtype=np.int64) * t["M"]) % t["L"]
    assert np.abs(yd).max() < 32767  # no clamp in play
    err = np.abs(y - yd)
    print(hz, "max err", err.max(), "max bound", bound.max())
    assert (err <= bound[ph] + 1e-6).all(), (err - bound[ph]).max()


def test_index_arithmetic_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_resample")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_resample.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
