"""The live-call entry points (tfp_live_*, tfp_group_live_*): exported by the library, declared in
the header with the reference lines they replace, bound in the ctypes mirror; the argument rules that
need no device; and the frame-range arithmetic of a push (csrc/tfp_live_plan.hpp) run stand-alone
under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (tests/native/check_live_plan.cpp). No GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import REPO

NEW_SYMBOLS = ["tfp_live_create", "tfp_live_destroy", "tfp_live_reset", "tfp_live_push", "tfp_live_samples",
               "tfp_live_stats", "tfp_group_live_create", "tfp_group_live_destroy", "tfp_group_live_reset",
               "tfp_group_live_push", "tfp_group_live_samples", "tfp_group_live_stats"]
TFP_E_ARG = -1


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    assert {"Live", "GroupLive"} <= set(dir(tfp_lib))
    for cls in (tfp_lib.Live, tfp_lib.GroupLive):
        for m in ("push", "reset", "samples", "stats"):
            assert callable(getattr(cls, m))


def test_header_section_cites_the_reference(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- live calls"):src.index("/* ---- device groups")]
    for cite in ("application_handler.c:152-185", ":248-312", "fp_handler.c:287-374", ":308-314",
                 "doc/dialplan_application.rst:11"):
        assert cite in sec, cite
    # every declaration of the section stands under a comment that names reference lines
    for m in re.finditer(r"^(?:int|void)\s+(tfp_live_[a-z_]+)\(", sec, re.M):
        above = sec[:m.start()]
        comment = above[above.rindex("/*"):]
        assert re.search(r"\.(?:c|rst):\d+", comment), m.group(1)


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    h = C.c_void_p()
    n = C.c_int64(7)
    assert lib.tfp_live_create(None, 8, 8000, 16000, C.byref(h)) == TFP_E_ARG and not h.value
    assert lib.tfp_live_create(None, 8, 8000, 16000, None) == TFP_E_ARG
    assert lib.tfp_live_reset(None, 0) == TFP_E_ARG
    assert lib.tfp_live_push(None, None, 160, None, None, None, 1, None, None, None) == TFP_E_ARG
    assert lib.tfp_live_samples(None, 0, C.byref(n)) == TFP_E_ARG and n.value == 7
    assert lib.tfp_live_stats(None, None, None, None, None, None) == TFP_E_ARG
    lib.tfp_live_destroy(None)
    assert lib.tfp_group_live_create(None, 8, 8000, 16000, C.byref(h)) == TFP_E_ARG and not h.value
    assert lib.tfp_group_live_reset(None, 0) == TFP_E_ARG
    assert lib.tfp_group_live_push(None, None, 160, None, None, None, 1, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_samples(None, 0, C.byref(n)) == TFP_E_ARG
    assert lib.tfp_group_live_stats(None, 0, None, None, None, None, None) == TFP_E_ARG
    lib.tfp_group_live_destroy(None)


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_live_plan_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_live_plan")
    subprocess.run(["g++", "-std=c++17", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_live_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
