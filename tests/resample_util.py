"""Shared by the rate-normalised ingest tests: the definition of tfp_resample.hpp restated in numpy (the
formula's taps in double, the int64 convolution over the library's own table), the frame comparison of
test_gpu_g711.py, and the inputs the tests share."""
import os
import re

import numpy as np

# the kernel's tile (outputs per workgroup), read where the kernel takes it from
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "asterisk-tiresias_amd", "csrc",
                       "tfp_resample.hpp")) as _f:
    TILE = int(re.search(r"constexpr int32_t kRsTile = (\d+);", _f.read()).group(1))

Z, BETA, RHO = 24, 8.0, 0.90
# (rate_in, rate_out): (L, M, ntaps)
PAIRS = {(16000, 8000): (1, 2, 97), (48000, 8000): (1, 6, 289), (96000, 8000): (1, 12, 577), (8000, 16000): (2, 1, 49),
         (44100, 8000): (80, 441, 266), (11025, 8000): (320, 441, 68), (44100, 48000): (160, 147, 49),
         (8001, 8000): (8000, 8001, 50)}


def plan(rate_in, rate_out):
    """(L, M, k_lo, k_hi) as defined."""
    g = int(np.gcd(rate_in, rate_out))
    L, M = rate_out // g, rate_in // g
    D = max(L, M)
    return L, M, -((Z * D) // L), -((-Z * D) // L)


def count(n_in, L, M):
    return 0 if n_in <= 0 else -((-n_in * L) // M)


def formula_taps(rate_in, rate_out):
    """h(u) in double per phase, each phase divided by its sum and multiplied by 32768: the unrounded table."""
    L, M, k_lo, k_hi = plan(rate_in, rate_out)
    D = max(L, M)
    k = np.arange(k_lo, k_hi + 1, dtype=np.int64)
    p = np.arange(L, dtype=np.int64)
    u = (k[None, :] * L - p[:, None]) / float(D)
    a = u / Z
    inside = np.abs(a) < 1.0
    w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - a * a, 0.0))) / np.i0(BETA)
    h = np.where(inside, RHO * np.sinc(RHO * u) * w, 0.0)
    return h / h.sum(axis=1, keepdims=True) * 32768.0


def convolve(x, t, taps=None):
    """The definition over the table t (resample_taps' dict): int64 sums, rounding and clamp -> int16; with
    taps (float, [L, ntaps]) the same sums in double, unrounded and unclamped, scaled by 2^-15."""
    x = np.asarray(x, np.int64)
    L, M, k_lo, nt = t["L"], t["M"], t["k_lo"], t["ntaps"]
    n_out = count(len(x), L, M)
    if n_out == 0:
        return np.zeros(0, np.int16 if taps is None else np.float64)
    n = np.arange(n_out, dtype=np.int64)
    i0, ph = (n * M) // L, (n * M) % L
    xp = np.concatenate([np.zeros(nt, np.int64), x, np.zeros(nt + 1, np.int64)])  # x = 0 outside the clip
    idx = (i0 + k_lo + nt)[:, None] + np.arange(nt, dtype=np.int64)[None, :]
    if taps is not None:
        return (taps[ph] * xp[idx]).sum(axis=1) / 32768.0
    acc = (t["taps"].astype(np.int64)[ph] * xp[idx]).sum(axis=1)
    return np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16)


def rails(n, M):
    """Full-scale alternation in runs of M samples."""
    return np.where((np.arange(n) // M) % 2 == 0, 32767, -32767).astype(np.int16)


def bits_equal(a, b):
    """Every field of two frame arrays, q1 and q2 as bit patterns (test_gpu_g711.py's _bits_equal)."""
    assert len(a) == len(b), (len(a), len(b))
    for k in ("frame_idx", "m1", "m2"):
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0][:10])
    for k in ("q1", "q2"):
        x, y = a[k].view(np.uint64), b[k].view(np.uint64)
        same = (x == y) | (np.isnan(a[k]) & np.isnan(b[k]))
        assert same.all(), (k, np.nonzero(~same)[0][:10])


def noise(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


def in_len_for(n_out, L, M):
    """The shortest input that gives at least n_out outputs (exactly n_out wherever some input does)."""
    n = max((n_out * M) // L - 1, 0)
    while count(n, L, M) < n_out:
        n += 1
    return n


def edge_lengths(t, tile):
    """Input lengths at which the conversion can go wrong: none, one, two, around the filter's length, and those
    that give tile - 1, tile, tile + 1 and 2 tile + 1 outputs."""
    L, M = t["L"], t["M"]
    return [0, 1, 2, t["ntaps"] - 1, t["ntaps"]] + [in_len_for(k, L, M) for k in (tile - 1, tile, tile + 1, 2 * tile + 1)]


def ragged_order(lens, seed=3):
    """lens three times over, in an order whose packed clip starts fall on every residue mod 8."""
    rng = np.random.default_rng(seed)
    lens = list(lens) * 3
    for _ in range(1000):
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        if set(int(s) % 8 for s in starts) == set(range(8)):
            return lens
        rng.shuffle(lens)
    raise AssertionError("no order covers every residue")


def class_clip(kind, n=24000):
    """A clip whose every frame lies in one box class of the reference's search (the integer parts of its
    two frame values, each value within 0.40 above its integer), before and after an 8 -> 16 -> 8 kHz round
    trip: kind 0 a 100 Hz tone (18, 17), kind 1 the same with noise of sigma 100 (17, 17), kind 2 a
    2000 Hz tone (19, 16)."""
    t = np.arange(n) / 8000.0
    f, sigma = ((100, 0), (100, 100), (2000, 0))[kind]
    x = 9000 * np.sin(2 * np.pi * f * t)
    if sigma:
        x = x + np.random.default_rng(f * 7 + sigma).normal(0, sigma, n)
    return np.rint(x).astype(np.int16)
