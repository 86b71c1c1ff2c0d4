"""The wide (int32 Q31) rate-normalised ingest entry points: exported by the library, declared in the header
under a section that states the definition, bound in the ctypes mirror; the argument rules that need no
device; the mirror's option. No GPU."""
import ctypes as C
import inspect
import re

NEW_SYMBOLS = ["tfp_wav_decode_interleaved_q31", "tfp_wav_read_interleaved_q31", "tfp_q31_from_f32", "tfp_q31_from_f64",
               "tfp_resample_wide_pcm", "tfp_fingerprint_wide_rate_batch", "tfp_search_wide_rate_batch",
               "tfp_search_scoped_wide_rate_batch", "tfp_resample_wide_stats", "tfp_group_fingerprint_wide_rate_batch",
               "tfp_group_search_wide_rate_batch", "tfp_group_search_scoped_wide_rate_batch"]
TFP_E_ARG = -1


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Engine, tfp_lib.Group):
        for m in ("resample_wide_pcm", "fingerprint_wide_rate_batch", "search_wide_rate_batch", "search_scoped_wide_rate_batch",
                  "resample_wide_stats"):
            assert callable(getattr(cls, m)), (cls, m)
    for f in ("resample_wide_pcm", "q31_from_float", "decode_wav_interleaved_q31", "read_wav_interleaved_q31"):
        assert callable(getattr(tfp_lib, f)), f
    sig = inspect.signature(tfp_lib.FpHandler.__init__)
    assert sig.parameters["wide_samples"].default is False and sig.parameters["mix_channels"].default is False


def test_header_states_the_definition(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- rate-normalised ingest of 24/32-bit and float audio"):
              src.index("/* ---- rate-normalised ingest of multichannel int16")]
    decls = re.findall(r"^int(?:32_t|64_t)?\s+(tfp_[a-z_0-9]+)\(", sec, re.M)
    assert sorted(decls) == sorted(NEW_SYMBOLS)
    for phrase in ("int32 Q31", "FRAMES", "floor((acc + 2^30 C) / (2^31 C))", "a floor, not a truncation",
                   "floor((S[i] + 2^15 C) / (2^16 C))", "tfp_resample_mix_pcm of x bit for bit", "A C >= 2^30",
                   "unsupported rate ratio", "(u - 128) << 24", "ties to even", "NaN 0", "NOT aubio's fp32 value",
                   "tfp_wav_decode_f32", "Not coalesced", "tfp_stream_push", "the compiled shim", "per-clip channel",
                   "packed 24-bit", "float-to-Q31 on the device"):
        assert phrase in sec, phrase
    # the two older sections point here instead of listing this input as uncovered
    mono = src[src.index("/* ---- rate-normalised ingest:"):src.index("/* ---- deterministic synthetic PCM")]
    mix = src[src.index("/* ---- rate-normalised ingest of multichannel int16"):src.index("/* ---- live calls at another rate")]
    assert "tfp_fingerprint_wide_rate_batch" in mono and "tfp_fingerprint_wide_rate_batch" in mix


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    from tiresias_amd import _lib
    p = tfp_lib.params(1, 0.45)
    off = (C.c_int64 * 2)(0, 0)
    n = C.c_int64(7)
    res = (_lib.Result * 1)()
    for ch in (1, 2):
        assert lib.tfp_fingerprint_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
        assert lib.tfp_search_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), res) == TFP_E_ARG
        assert lib.tfp_search_scoped_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), None, 1, None, None,
                                                     None) == TFP_E_ARG
        assert lib.tfp_group_fingerprint_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
        assert lib.tfp_group_search_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), res) == TFP_E_ARG
        assert lib.tfp_group_search_scoped_wide_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), None, 1, None, None,
                                                           None) == TFP_E_ARG
    assert lib.tfp_resample_wide_stats(None, None, None, None, None) == TFP_E_ARG
    assert n.value == 7
