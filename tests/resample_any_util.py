"""Shared by the mixed-batch tests: the staging constants read where the kernels take them from, the existing host
map of each class (the definition of a mixed clip), and clips of every class."""
import os
import re

import numpy as np

from resample_util import TILE, count

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "asterisk-tiresias_amd", "csrc",
                       "tfp_resample.hpp")) as _f:
    _src = _f.read()
SPAN_MAX_I16 = int(re.search(r"constexpr int32_t kRsSpanMax = (\d+);", _src).group(1))      # int16 mono, G.711
SPAN_MAX_MIX = int(re.search(r"constexpr int32_t kRsMixSpanMax = (\d+);", _src).group(1))   # int32 sums, Q31 mono
SPAN_MAX_WIDE = int(re.search(r"constexpr int32_t kRsWideSpanMax = (\d+);", _src).group(1))  # int64 sums

S16, Q31, ULAW, ALAW = 0, 1, 2, 3
DTYPE = {S16: np.int16, Q31: np.int32, ULAW: np.uint8, ALAW: np.uint8}


def samples(kind, nframes, ch, seed):
    """Noise over the kind's whole range, [nframes, ch]."""
    rng = np.random.default_rng(seed)
    if kind == S16:
        return rng.integers(-32768, 32768, (nframes, ch)).astype(np.int16)
    if kind == Q31:
        return rng.integers(-2**31, 2**31, (nframes, ch)).astype(np.int32)
    return rng.integers(0, 256, (nframes, ch)).astype(np.uint8)


def class_map(T, x, kind, rate_in, rate_out):
    """The existing host map of the clip's class: what a mixed clip is defined to be."""
    ch = x.shape[1]
    if kind == S16:
        return T.resample_pcm(x.reshape(-1), rate_in, rate_out) if ch == 1 else T.resample_mix_pcm(x, ch, rate_in, rate_out)
    if kind == Q31:
        return T.resample_wide_pcm(x, ch, rate_in, rate_out)
    return T.resample_pcm(T.decode_g711(x.reshape(-1), kind - ULAW), rate_in, rate_out)


def form_of(T, kind, ch, rate_in, rate_out):
    """'plain', 'staged' or 'global': the clip's class's own staging rule over the pair's span."""
    if rate_in == rate_out:
        return "plain"
    t = T.resample_taps(rate_in, rate_out)
    span = ((TILE - 1) * t["M"]) // t["L"] + 1 + t["ntaps"]
    limit = SPAN_MAX_I16 if kind in (ULAW, ALAW) or (kind == S16 and ch == 1) else \
        SPAN_MAX_MIX if kind == S16 or ch == 1 else SPAN_MAX_WIDE
    return "staged" if span <= limit else "global"


def tiles(n_out):
    return -(-n_out // TILE)


def out_len(nframes, rate_in, rate_out):
    g = int(np.gcd(rate_in, rate_out))
    return nframes if rate_in == rate_out else count(nframes, rate_out // g, rate_in // g)


def uuid(c):
    return "%08x-a11c-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


def key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def render(tfp_lib, clip, cls, seed):
    """An 8 kHz int16 clip re-rendered in one of four classes: (samples, rate_in, kind)."""
    rng = np.random.default_rng(seed)
    if cls == 0:  # int16 mono at 16000
        return tfp_lib.resample_pcm(clip, 8000, 16000).reshape(-1, 1), 16000, S16
    if cls == 1:  # int16 stereo at 44100: the clip plus and minus a difference signal
        up = tfp_lib.resample_pcm(clip, 8000, 44100).astype(np.int32)
        side = rng.integers(-200, 201, len(up))
        return np.clip(np.stack([up + side, up - side], 1), -32768, 32767).astype(np.int16), 44100, S16
    if cls == 2:  # Q31 stereo at 48000, the 16 bits below an int16 step filled
        up = tfp_lib.resample_pcm(clip, 8000, 48000).astype(np.int64) << 16
        fine = rng.integers(-2**15, 2**15, (len(up), 2))
        return np.clip(up[:, None] + fine, -2**31, 2**31 - 1).astype(np.int32), 48000, Q31
    return clip.reshape(-1, 1).astype(np.int16), 8000, S16  # int16 mono at the index rate (plain)
