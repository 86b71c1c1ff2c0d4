"""The rate-normalised ingest entry points: exported by the library, declared in the header under comments
that say what each equals, bound in the ctypes mirror; and the argument rules that need no device. No GPU."""
import ctypes as C
import re

NEW_SYMBOLS = ["tfp_resample_count", "tfp_resample_taps", "tfp_resample_pcm", "tfp_fingerprint_rate_batch", "tfp_search_rate_batch", "tfp_search_scoped_rate_batch", "tfp_resample_stats",
               "tfp_group_fingerprint_rate_batch", "tfp_group_search_rate_batch", "tfp_group_search_scoped_rate_batch"]
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
        for m in ("resample_count", "resample_taps", "resample_pcm", "fingerprint_rate_batch", "search_rate_batch",
                  "search_scoped_rate_batch", "resample_stats"):
            assert callable(getattr(cls, m)), (cls, m)


def test_header_says_what_each_form_equals(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- rate-normalised ingest"):src.index("/* ---- deterministic synthetic PCM")]
    decls = re.findall(r"^int(?:32_t|64_t)?\s+(tfp_[a-z_0-9]+)\(", sec, re.M)
    assert sorted(decls) == sorted(NEW_SYMBOLS)
    for phrase in ("fp_handler.c:37", "bad sample rate", "unsupported rate ratio", "tfp_fingerprint_batch at rate_out",
                   "tfp_search_pcm_batch at rate_out", "tfp_search_scoped_pcm_batch at rate_out", "tfp_resample_pcm",
                   "tfp_stream_push", "fp32"):
        assert phrase in sec, phrase


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    from tiresias_amd import _lib
    p = tfp_lib.params(1, 0.45)
    off = (C.c_int64 * 2)(0, 0)
    n = C.c_int64(7)
    res = (_lib.Result * 1)()
    assert lib.tfp_fingerprint_rate_batch(None, None, off, 1, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
    assert lib.tfp_search_rate_batch(None, None, off, 1, 16000, 8000, C.byref(p), res) == TFP_E_ARG
    assert lib.tfp_search_scoped_rate_batch(None, None, off, 1, 16000, 8000, C.byref(p), None, 1, None, None, None) == TFP_E_ARG
    assert lib.tfp_resample_stats(None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_fingerprint_rate_batch(None, None, off, 1, 16000, 8000, None, 0, C.byref(n)) == TFP_E_ARG
    assert lib.tfp_group_search_rate_batch(None, None, off, 1, 16000, 8000, C.byref(p), res) == TFP_E_ARG
    assert lib.tfp_group_search_scoped_rate_batch(None, None, off, 1, 16000, 8000, C.byref(p), None, 1, None, None,
                                                  None) == TFP_E_ARG
    assert n.value == 7
