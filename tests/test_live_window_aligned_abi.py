"""The aligned trailing-window entry points of live calls (tfp_live_window_aligned,
tfp_live_window_aligned_stats and their tfp_group_live_* forms): exported by the library, declared in the
header under comments that cite the reference lines, bound in the ctypes mirror, and the argument rules
that need no device. No GPU."""
import ctypes as C
import re

NEW_SYMBOLS = ["tfp_live_window_aligned", "tfp_live_window_aligned_stats", "tfp_group_live_window_aligned",
               "tfp_group_live_window_aligned_stats"]
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
        for m in ("window_aligned", "window_aligned_stats"):
            assert callable(getattr(cls, m))


def test_header_declarations_cite_the_reference(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* The aligned trailing window"):src.index("/* ---- device groups")]
    for name in NEW_SYMBOLS[:2]:
        m = re.search(r"^int\s+%s\(" % name, sec, re.M)
        assert m, name
        above = sec[:m.start()]
        comment = above[above.rindex("/*"):]
        assert re.search(r"\.(?:c|rst):\d+", comment), name
    for cite in ("application_handler.c:152-185", ":248-312", "fp_handler.c:287-351", ":367-374", "clip_start_frame"):
        assert cite in sec, cite
    grp = src[src.index("/* tfp_live_window_aligned on a group"):]
    for name in NEW_SYMBOLS[2:]:
        assert re.search(r"^int\s+%s\(" % name, grp, re.M), name
    assert re.search(r"\.c:\d+", grp[:grp.index("*/")])


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    p = tfp_lib.params(1, 0.45)
    cnt = (C.c_int32 * 1)(5)
    out = (tfp_lib.engine.Candidate * 1)()
    al = (tfp_lib.engine.Alignment * 1)()
    # a NULL handle, and a NULL align on a NULL handle: TFP_E_ARG, the sentinel stays
    for fn in (lib.tfp_live_window_aligned, lib.tfp_group_live_window_aligned):
        assert fn(None, C.byref(p), None, 1, 1, out, al, cnt, None, None) == TFP_E_ARG and cnt[0] == 5
        assert fn(None, C.byref(p), None, 1, 1, out, None, cnt, None, None) == TFP_E_ARG and cnt[0] == 5
    assert lib.tfp_live_window_aligned_stats(None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_window_aligned_stats(None, 0, None, None, None) == TFP_E_ARG
