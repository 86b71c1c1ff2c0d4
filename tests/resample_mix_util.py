"""Shared by the multichannel rate-normalised ingest tests: the definition of tfp_resample.hpp's multichannel
form restated in numpy (int64 channel sums, resample_util.convolve's index arithmetic, Python's floor
division), the kernel's staging budget read where the kernel takes it from, and the inputs the tests share."""
import os
import re

import numpy as np

from resample_util import count

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "asterisk-tiresias_amd", "csrc",
                       "tfp_resample.hpp")) as _f:
    _src = _f.read()
    SPAN_MAX = int(re.search(r"constexpr int32_t kRsMixSpanMax = (\d+);", _src).group(1))
    CHANNELS_MAX = int(re.search(r"constexpr int32_t kRsMixChannelsMax = (\d+);", _src).group(1))


def mix_convolve(x, t):
    """x int16[nframes, C], t resample_taps' dict -> int16[n_out]: S = sum over channels (int64), the exact sum
    over the taps, floor((acc + 16384 C) / (32768 C)), clamp."""
    x = np.asarray(x, np.int64)
    C = x.shape[1]
    S = x.sum(axis=1)
    L, M, k_lo, nt = t["L"], t["M"], t["k_lo"], t["ntaps"]
    n_out = count(len(S), L, M)
    if n_out == 0:
        return np.zeros(0, np.int16)
    n = np.arange(n_out, dtype=np.int64)
    i0, ph = (n * M) // L, (n * M) % L
    sp = np.concatenate([np.zeros(nt, np.int64), S, np.zeros(nt + 1, np.int64)])  # S = 0 outside the clip
    idx = (i0 + k_lo + nt)[:, None] + np.arange(nt, dtype=np.int64)[None, :]
    acc = (t["taps"].astype(np.int64)[ph] * sp[idx]).sum(axis=1)
    return np.clip((acc + 16384 * C) // (32768 * C), -32768, 32767).astype(np.int16)  # numpy's // floors


def mix_mean(x):
    """Equal rates: floor((2 S + C) / (2 C)) per frame."""
    x = np.asarray(x, np.int64)
    C = x.shape[1]
    return ((2 * x.sum(axis=1) + C) // (2 * C)).astype(np.int16)


def mix_noise(nframes, C, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (nframes, C)).astype(np.int16)


def span_max(t, tile):
    """The most frames a tile of `tile` outputs spans (the kernel's own bound)."""
    return ((tile - 1) * t["M"]) // t["L"] + 1 + t["ntaps"]


def pack(clips, C):
    """Clips int16[nframes_i, C] -> (flat interleaved samples, offsets in frames)."""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    flat = np.concatenate([np.asarray(c, np.int16).reshape(-1) for c in clips]) if clips else np.zeros(0, np.int16)
    return flat.astype(np.int16), off
