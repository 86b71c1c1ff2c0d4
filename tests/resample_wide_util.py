"""Shared by the wide (int32 Q31) rate-normalised ingest tests: the definition of tfp_resample.hpp's wide form
restated in Python big integers (numpy object arrays: no width to overflow), the kernel's two staging limits
read where the kernel takes them from, and the inputs the tests share."""
import os
import re

import numpy as np

from resample_util import count

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "asterisk-tiresias_amd", "csrc",
                       "tfp_resample.hpp")) as _f:
    _src = _f.read()
    SPAN_MAX_MONO = int(re.search(r"constexpr int32_t kRsMixSpanMax = (\d+);", _src).group(1))   # int32 samples, C = 1
    SPAN_MAX_SUMS = int(re.search(r"constexpr int32_t kRsWideSpanMax = (\d+);", _src).group(1))  # int64 sums, C >= 2

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def _floor_clamp(num, den):
    return np.array([min(max(int(a) // den, -32768), 32767) for a in num], np.int16)  # Python's // floors


def wide_convolve(q, t):
    """q int32[nframes, C], t resample_taps' dict -> int16[n_out]: S = sum over channels, the exact sum over the
    taps, floor((acc + 2^30 C) / (2^31 C)), clamp; every product and sum a Python integer."""
    q = np.asarray(q).astype(object)
    C = q.shape[1]
    S = q.sum(axis=1) if len(q) else np.zeros(0, object)
    L, M, k_lo, nt = t["L"], t["M"], t["k_lo"], t["ntaps"]
    n_out = count(len(S), L, M)
    if n_out == 0:
        return np.zeros(0, np.int16)
    n = np.arange(n_out, dtype=np.int64)
    i0, ph = (n * M) // L, (n * M) % L
    sp = np.concatenate([np.zeros(nt, object), S, np.zeros(nt + 1, object)])  # S = 0 outside the clip
    idx = (i0 + k_lo + nt)[:, None] + np.arange(nt, dtype=np.int64)[None, :]
    acc = (t["taps"].astype(object)[ph] * sp[idx]).sum(axis=1)
    return _floor_clamp(acc + 2**30 * C, 2**31 * C)


def wide_mean(q):
    """Equal rates: clamp(floor((S + 2^15 C) / (2^16 C))) per frame."""
    q = np.asarray(q).astype(object)
    C = q.shape[1]
    if not len(q):
        return np.zeros(0, np.int16)
    return _floor_clamp(q.sum(axis=1) + 2**15 * C, 2**16 * C)


def wide_reference(q, t, rate_in, rate_out):
    return wide_mean(q) if rate_in == rate_out else wide_convolve(q, t)


def wide_noise(nframes, C, seed):
    return np.random.default_rng(seed).integers(INT32_MIN, INT32_MAX + 1, (nframes, C)).astype(np.int32)


def abs_sum(t):
    """A = max over the phases of the sum of |tap|."""
    return int(np.abs(t["taps"].astype(np.int64)).sum(axis=1).max())


def span_max(t, tile):
    """The most frames a tile of `tile` outputs spans (the kernel's own bound)."""
    return ((tile - 1) * t["M"]) // t["L"] + 1 + t["ntaps"]


def pack(clips, C):
    """Clips int32[nframes_i, C] -> (flat interleaved samples, offsets in frames)."""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    flat = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in clips]) if clips else np.zeros(0, np.int32)
    return flat.astype(np.int32), off
