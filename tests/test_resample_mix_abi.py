"""The multichannel rate-normalised ingest entry points: exported by the library, declared in the header
under a section that states the definition, bound in the ctypes mirror; the argument rules that need no
device. No GPU."""
import ctypes as C
import re

NEW_SYMBOLS = ["tfp_wav_decode_interleaved", "tfp_wav_read_interleaved", "tfp_resample_mix_pcm",
               "tfp_fingerprint_mix_rate_batch", "tfp_search_mix_rate_batch", "tfp_search_scoped_mix_rate_batch",
               "tfp_resample_mix_stats", "tfp_group_fingerprint_mix_rate_batch", "tfp_group_search_mix_rate_batch",
               "tfp_group_search_scoped_mix_rate_batch"]
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
        for m in ("resample_mix_pcm", "fingerprint_mix_rate_batch", "search_mix_rate_batch", "search_scoped_mix_rate_batch",
                  "resample_mix_stats"):
            assert callable(getattr(cls, m)), (cls, m)
    for f in ("resample_mix_pcm", "decode_wav_interleaved", "read_wav_interleaved"):
        assert callable(getattr(tfp_lib, f)), f
    assert tfp_lib.MIX_CHANNELS_MAX == 32


def test_header_states_the_definition(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- rate-normalised ingest of multichannel int16"):src.index("/* ---- live calls at another rate")]
    decls = re.findall(r"^int(?:32_t|64_t)?\s+(tfp_[a-z_0-9]+)\(", sec, re.M)
    assert sorted(decls) == sorted(NEW_SYMBOLS)
    assert re.search(r"#define TFP_MIX_CHANNELS_MAX 32\b", sec)
    for phrase in ("FRAMES", "floor((acc + 16384 C) / (32768 C))", "a floor, not a truncation", "tfp_resample_pcm bit for bit",
                   "floor((2 S[i] + C) / (2 C))", "NOT aubio's fp32 channel mean", "tfp_wav_decode_f32",
                   "unsupported channel count", "Not coalesced", "tfp_resample_stats", "24/32-bit and float input",
                   "tfp_stream_push", "the compiled shim", "per-clip channel counts"):
        assert phrase in sec, phrase


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    from tiresias_amd import _lib
    p = tfp_lib.params(1, 0.45)
    off = (C.c_int64 * 2)(0, 0)
    n = C.c_int64(7)
    res = (_lib.Result * 1)()
    for ch in (1, 2):
        assert lib.tfp_fingerprint_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
        assert lib.tfp_search_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), res) == TFP_E_ARG
        assert lib.tfp_search_scoped_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), None, 1, None, None,
                                                    None) == TFP_E_ARG
        assert lib.tfp_group_fingerprint_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
        assert lib.tfp_group_search_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), res) == TFP_E_ARG
        assert lib.tfp_group_search_scoped_mix_rate_batch(None, None, off, 1, ch, 16000, 8000, C.byref(p), None, 1, None, None,
                                                          None) == TFP_E_ARG
    assert lib.tfp_resample_mix_stats(None, None, None, None, None) == TFP_E_ARG
    assert n.value == 7
