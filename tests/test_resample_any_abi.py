"""The mixed-batch entry points: exported by the library, declared in the header under a section of their own that
states the definition and what stays out of scope, bound in the ctypes mirror; every argument rule that needs no
device, with the offending clip's index in the message; the mirror's option. No GPU."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

NEW_SYMBOLS = ["tfp_resample_any_pcm", "tfp_audio_clips_check", "tfp_fingerprint_any_batch", "tfp_search_any_batch",
               "tfp_search_scoped_any_batch", "tfp_resample_any_stats", "tfp_group_fingerprint_any_batch",
               "tfp_group_search_any_batch", "tfp_group_search_scoped_any_batch"]
TFP_E_ARG = -1
S16, Q31, ULAW, ALAW = 0, 1, 2, 3


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Engine, tfp_lib.Group):
        for m in ("resample_any_pcm", "fingerprint_any_batch", "search_any_batch", "search_scoped_any_batch", "resample_any_stats"):
            assert callable(getattr(cls, m)), (cls, m)
    for f in ("resample_any_pcm", "audio_clips_check", "pack_audio_clips"):
        assert callable(getattr(tfp_lib, f)), f
    assert (tfp_lib.AUDIO_S16, tfp_lib.AUDIO_Q31, tfp_lib.AUDIO_ULAW, tfp_lib.AUDIO_ALAW) == (S16, Q31, ULAW, ALAW)
    assert tfp_lib.CLIP_DTYPE.itemsize == 32 and tfp_lib.ANY_RATES_MAX == 64
    assert inspect.signature(tfp_lib.FpHandler.__init__).parameters["mixed_batch"].default is False


def test_header_section(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    # between the misc section and the 24/32-bit section, under a title the older sections' slices do not match
    a, b = src.index("/* ---- mixed batches: clips of any rate"), src.index("/* ---- rate-normalised ingest of 24/32-bit")
    assert src.index("/* ---- misc") < a < b
    sec = src[a:b]
    decls = re.findall(r"^int(?:32_t|64_t)?\s+(tfp_[a-z_0-9]+)\(", sec, re.M)
    assert sorted(decls) == sorted(NEW_SYMBOLS)
    for phrase in ("TFP_AUDIO_S16 = 0, TFP_AUDIO_Q31 = 1, TFP_AUDIO_ULAW = 2, TFP_AUDIO_ALAW = 3", "#define TFP_ANY_RATES_MAX 64",
                   "typedef struct tfp_audio_clip", "BYTES", "tfp_resample_pcm", "tfp_resample_mix_pcm", "tfp_resample_wide_pcm",
                   "tfp_g711_decode", "ONE launch", "all-or-nothing", "bad sample rate", "unsupported rate ratio", "A C >= 2^30",
                   "Not coalesced", "float-to-Q31", "packed 24-bit", "taps in LDS", "tfp_stream_push", "query-sharded",
                   "coalescing"):
        assert phrase in sec, phrase


def _clip(offset=0, nframes=10, rate_in=16000, channels=1, kind=S16, reserved=0):
    return (offset, nframes, rate_in, channels, kind, reserved)


RULES = [(_clip(rate_in=0), "bad sample rate"), (_clip(rate_in=-8000), "bad sample rate"),
         (_clip(rate_in=7999, kind=Q31), "unsupported rate ratio 7999 -> 44100"),
         (_clip(channels=0), "unsupported channel count"), (_clip(channels=33), "unsupported channel count"),
         (_clip(channels=2, kind=ULAW), "G.711 of 2 channels"), (_clip(channels=2, kind=ALAW), "G.711 of 2 channels"),
         (_clip(kind=4), "unknown sample kind"), (_clip(kind=-1), "unknown sample kind"), (_clip(reserved=1), "reserved"),
         (_clip(offset=1), "multiple of the sample size"), (_clip(offset=2, kind=Q31), "multiple of the sample size"),
         (_clip(offset=-2), "multiple of the sample size"), (_clip(nframes=-1), "negative frame count"),
         (_clip(offset=4000, nframes=49), "reaches past"), (_clip(offset=4098, nframes=0), "reaches past"),
         (_clip(nframes=2**62, channels=32, kind=Q31), "reaches past")]


@pytest.mark.parametrize("clip,msg", RULES, ids=[m.replace(" ", "-") + str(i) for i, (_, m) in enumerate(RULES)])
def test_argument_rules_name_the_first_offending_clip(tfp_lib, clip, msg):
    rate_out = 44100 if "7999" in msg else 8000
    good = [_clip(), _clip(offset=100, kind=ULAW, rate_in=8000), _clip(offset=8, kind=Q31, channels=2, rate_in=44100)]
    for at in (0, 2, 3):
        clips = good[:at] + [clip] + good[at:] + [_clip(kind=9)]  # a later offender is not the one named
        with pytest.raises(tfp_lib.TfpError) as ei:
            tfp_lib.audio_clips_check(clips, 4096, rate_out)
        assert ei.value.code == TFP_E_ARG and "clip %d: " % at in str(ei.value) and msg in str(ei.value), str(ei.value)
    assert list(tfp_lib.audio_clips_check(good, 4096, 8000)) == [5, 10, 2]


def test_rate_rules_and_the_rate_limit(tfp_lib):
    with pytest.raises(tfp_lib.TfpError, match="bad sample rate 0"):
        tfp_lib.audio_clips_check([_clip()], 4096, 0)
    many = [_clip(rate_in=8000 + 8 * i) for i in range(65)]          # the index rate itself counts as one
    assert len(tfp_lib.audio_clips_check(many[:64], 4096, 8000)) == 64
    with pytest.raises(tfp_lib.TfpError, match="clip 64: more than 64 distinct input rates"):
        tfp_lib.audio_clips_check(many, 4096, 8000)
    assert len(tfp_lib.audio_clips_check(many[:64] + many[:64], 4096, 8000)) == 128  # a rate met before is no new rate
    # G.711 has no per-tap form: a reduction past the int16 staging limit is refused, int16 at the same pair is not
    assert len(tfp_lib.audio_clips_check([_clip(rate_in=256000)], 4096, 8000)) == 1
    with pytest.raises(tfp_lib.TfpError, match="clip 0: unsupported rate ratio 256000 -> 8000 for G.711"):
        tfp_lib.audio_clips_check([_clip(rate_in=256000, kind=ULAW)], 4096, 8000)
    # the one-clip host map gives the same refusals
    with pytest.raises(tfp_lib.TfpError, match="clip 0: G.711 of 2 channels"):
        tfp_lib.resample_any_pcm(np.zeros(64, np.uint8), _clip(channels=2, kind=ULAW), 8000)


def test_null_handles(tfp_lib):
    lib = tfp_lib.lib()
    from tiresias_amd import _lib
    p = tfp_lib.params(1, 0.45)
    clips = np.zeros(1, tfp_lib.CLIP_DTYPE)
    n = C.c_int64(7)
    res = (_lib.Result * 1)()
    for pfx in ("tfp_", "tfp_group_"):
        assert getattr(lib, pfx + "fingerprint_any_batch")(None, None, 0, clips.ctypes.data, 1, 8000, None, 0, C.byref(n)) == TFP_E_ARG
        assert getattr(lib, pfx + "search_any_batch")(None, None, 0, clips.ctypes.data, 1, 8000, C.byref(p), res) == TFP_E_ARG
        assert getattr(lib, pfx + "search_scoped_any_batch")(None, None, 0, clips.ctypes.data, 1, 8000, C.byref(p), None, 1, None,
                                                             None, None) == TFP_E_ARG
    assert lib.tfp_resample_any_stats(None, *([None] * 7)) == TFP_E_ARG
    assert n.value == 7
