"""The trailing-window entry points of live calls (tfp_live_window, tfp_live_frames, tfp_live_window_stats
and their tfp_group_live_* forms): exported by the library, declared in the header under comments that
cite the reference lines, bound in the ctypes mirror; the argument rules that need no device; and the
window's frame-range arithmetic (csrc/tfp_live_window.hpp) run stand-alone under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU (tests/native/check_live_window.cpp). No GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import REPO

NEW_SYMBOLS = ["tfp_live_window", "tfp_live_frames", "tfp_live_window_stats", "tfp_group_live_window",
               "tfp_group_live_frames", "tfp_group_live_window_stats"]
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
        for m in ("window", "frames", "window_stats"):
            assert callable(getattr(cls, m))


def test_header_declarations_cite_the_reference(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- live calls"):src.index("/* ---- device groups")]
    for name in NEW_SYMBOLS[:3]:
        m = re.search(r"^int\s+%s\(" % name, sec, re.M)
        assert m, name
        above = sec[:m.start()]
        comment = above[above.rindex("/*"):]
        assert re.search(r"\.(?:c|rst):\d+", comment), name
    for cite in ("application_handler.c:152-185", ":248-312", "fp_handler.c:287-374", ":308-314"):
        assert cite in sec[sec.index("/* The trailing window"):], cite
    grp = src[src.index("/* tfp_live_window on a group"):]
    for name in NEW_SYMBOLS[3:]:
        assert re.search(r"^int\s+%s\(" % name, grp, re.M), name
    assert re.search(r"\.c:\d+", grp[:grp.index("*/")])


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    n = C.c_int64(7)
    p = tfp_lib.params(1, 0.45)
    cnt = (C.c_int32 * 1)(5)
    assert lib.tfp_live_window(None, C.byref(p), None, 1, 1, None, cnt, None, None) == TFP_E_ARG and cnt[0] == 5
    assert lib.tfp_live_frames(None, 0, 0, None, 0, C.byref(n)) == TFP_E_ARG and n.value == 7
    assert lib.tfp_live_window_stats(None, None, None, None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_window(None, C.byref(p), None, 1, 1, None, cnt, None, None) == TFP_E_ARG and cnt[0] == 5
    assert lib.tfp_group_live_frames(None, 0, 0, None, 0, C.byref(n)) == TFP_E_ARG and n.value == 7
    assert lib.tfp_group_live_window_stats(None, 0, None, None, None, None, None, None) == TFP_E_ARG
    # window_ms in frames: ceil(window_ms * rate / 1000 / 256), at least 1 (host-only)
    assert hasattr(lib, "tfp_live_window_frames") and "tfp_live_window_frames" in tfp_lib.header_symbols()
    for ms, rate, frames in ((32, 8000, 1), (33, 8000, 2), (2000, 8000, 63), (2000, 16000, 125), (1, 8000, 1), (0, 8000, 1),
                             (-5, 8000, 1), (16, 16000, 1), (17, 16000, 2)):
        assert lib.tfp_live_window_frames(ms, rate) == frames, (ms, rate)


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_live_window_plan_asan_ubsan(tmp_path):
    """Every S in [0, 2600] reached by ticks of 1, 160, 255, 256, 257 and 1,000 samples, windows of 1, 2, 3,
    7 and 100 frames, a window call after every push or after every few: the plan's ranges equal the set
    differences of row and target, restart is chosen exactly when it visits fewer frames, and the
    visited count never exceeds min(leaving + entering, target)."""
    exe = str(tmp_path / "check_live_window")
    subprocess.run(["g++", "-std=c++17", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_live_window.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
