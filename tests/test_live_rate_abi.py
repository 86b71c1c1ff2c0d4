"""The entry points of a live object with an input rate (tfp_live_create_rate and its group twins): exported
by the library, declared in the header's last section under comments that state the contract and name the
reference lines, bound in the ctypes mirror; and the argument rules that need no device. No GPU."""
import ctypes as C
import re

NEW_SYMBOLS = ["tfp_live_create_rate", "tfp_live_input_samples", "tfp_live_rate_info", "tfp_live_rate_stats",
               "tfp_group_live_create_rate", "tfp_group_live_input_samples", "tfp_group_live_rate_info",
               "tfp_group_live_rate_stats"]
TFP_E_ARG = -1


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Live, tfp_lib.GroupLive):
        for m in ("input_samples", "rate_info", "rate_stats", "finish"):
            assert callable(getattr(cls, m)), (cls, m)


def test_header_section_states_the_contract(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- live calls at another rate"):]
    assert src.index("/* ---- live calls at another rate") > src.index("/* ---- misc")  # the header's last section
    decls = re.findall(r"^int\s+(tfp_[a-z_0-9]+)\(", sec, re.M)
    assert sorted(decls) == sorted(NEW_SYMBOLS)
    for phrase in ("i0 + k_hi <= S_in - 1", "tfp_resample_count(S_in - k_hi)", "0 while S_in <= k_hi",
                   "48 at 16000 -> 8000", "144 at 48000 -> 8000", "24 at 8000 -> 16000", "133 at 44100 -> 8000", "3 ms",
                   "ntaps - 1 input samples", "k_hi zero samples", "tfp_resample_count(S_in)", "zero flush",
                   "bad sample rate", "unsupported rate ratio", "TFP_E_CAPACITY", "one object per rate"):
        assert phrase in sec, phrase
    # every declaration of the section stands under a comment that names reference lines
    for m in re.finditer(r"^int\s+(tfp_(?:group_)?live_[a-z_]+)\(", sec, re.M):
        above = sec[:m.start()]
        comment = above[above.rindex("/*"):]
        assert re.search(r"\.(?:c|rst):\d+", comment), m.group(1)
    # the batch section no longer names the live forms as uncovered, and points here
    batch = src[src.index("/* ---- rate-normalised ingest"):src.index("/* ---- deterministic synthetic PCM")]
    assert "tfp_live_create_rate" in batch and "tfp_stream_push / tfp_live_push" not in batch


def test_null_handles_are_refused_and_write_nothing(tfp_lib):
    lib = tfp_lib.lib()
    h = C.c_void_p()
    n, a, b, c = C.c_int64(7), C.c_int64(7), C.c_int64(7), C.c_int64(7)
    r = C.c_int32(7)
    for pfx in ("tfp_live", "tfp_group_live"):
        fn = lambda name: getattr(lib, pfx + name)
        assert fn("_create_rate")(None, 8, 16000, 8000, 16000, C.byref(h)) == TFP_E_ARG and not h.value
        assert fn("_create_rate")(None, 8, 16000, 8000, 16000, None) == TFP_E_ARG
        assert fn("_input_samples")(None, 0, C.byref(n)) == TFP_E_ARG and n.value == 7
        assert fn("_rate_info")(None, C.byref(r), C.byref(n)) == TFP_E_ARG and (r.value, n.value) == (7, 7)
    assert lib.tfp_live_rate_stats(None, C.byref(a), C.byref(b), C.byref(c)) == TFP_E_ARG
    assert lib.tfp_group_live_rate_stats(None, 0, C.byref(a), C.byref(b), C.byref(c)) == TFP_E_ARG
    assert (a.value, b.value, c.value) == (7, 7, 7)
