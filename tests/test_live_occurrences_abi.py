"""The occurrence entry points of live calls (tfp_live_occurrences, tfp_live_tracks, tfp_live_occurrence_stats
and their tfp_group_live_* forms): exported by the library, declared in the header with the documented
signatures under comments that cite the reference lines, bound in the ctypes mirror; the argument rules
that need no device; and the carry argument (a stored trace summary extended by the frames that became
final equals the one-shot trace) stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer on the
CPU (tests/native/check_live_trace.cpp). No GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import REPO

NEW_SYMBOLS = ["tfp_live_occurrences", "tfp_live_tracks", "tfp_live_occurrence_stats", "tfp_group_live_occurrences",
               "tfp_group_live_tracks", "tfp_group_live_occurrence_stats"]
TFP_E_ARG = -1
OCC_ARGS = ("const tfp_search_params* params, const int32_t* scopes, int32_t k, int32_t window, int32_t max_gap, "
            "int32_t min_hits, int32_t max_tracks, tfp_occurrence* out, int64_t cap, int64_t* noccurrences, int32_t* dropped")
TRACK_ARGS = "int32_t channel, tfp_trace_req* reqs, tfp_trace* traces, int32_t* windows, int64_t cap, int64_t* ntracks"
STAT_ARGS = "int64_t* calls, int64_t* tracks_added, int64_t* tracks_dropped, int64_t* frames_traced, int64_t* retraces"
SIGNATURES = {
    "tfp_live_occurrences": "tfp_live* lv, " + OCC_ARGS,
    "tfp_live_tracks": "tfp_live* lv, " + TRACK_ARGS,
    "tfp_live_occurrence_stats": "tfp_live* lv, " + STAT_ARGS,
    "tfp_group_live_occurrences": "tfp_group_live* lv, " + OCC_ARGS,
    "tfp_group_live_tracks": "tfp_group_live* lv, " + TRACK_ARGS,
    "tfp_group_live_occurrence_stats": "tfp_group_live* lv, int32_t shard, " + STAT_ARGS,
}


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Live, tfp_lib.GroupLive):
        for m in ("occurrences", "tracks", "occurrence_stats"):
            assert callable(getattr(cls, m))


def _norm(s):
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"\s+", " ", s).strip()


def test_header_signatures_and_citations(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    for name, args in SIGNATURES.items():
        m = re.search(r"^int\s+%s\((.*?)\);" % name, src, re.M | re.S)
        assert m, name
        assert _norm(m.group(1)) == args, (name, _norm(m.group(1)))
        assert len(_lib._SIGS[name][1]) == args.count(",") + 1, name
    sec = src[src.index("/* The log of a live call"):src.index("/* ---- device groups")]
    for name in NEW_SYMBOLS[:3]:
        m = re.search(r"^int\s+%s\(" % name, sec, re.M)
        above = sec[:m.start()]
        assert re.search(r"\.(?:c|rst):\d+", above[above.rindex("/*"):]), name
    for cite in ("application_handler.c:152-185", "fp_handler.c:287-351", ":367-374", "TFP_LIVE_TRACKS_MAX", "max_tracks"):
        assert cite in sec, cite
    m = re.search(r"^#define\s+TFP_LIVE_TRACKS_MAX\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) >= 64
    grp = src[src.index("/* tfp_live_occurrences on a group"):]
    assert re.search(r"\.c:\d+", grp[:grp.index("*/")])


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    p = tfp_lib.params(1, 0.45)
    n = C.c_int64(77)
    drop = (C.c_int32 * 1)(5)
    out = (tfp_lib.engine.Occurrence * 1)()
    out[0].hits = 9
    for fn in (lib.tfp_live_occurrences, lib.tfp_group_live_occurrences):
        assert fn(None, C.byref(p), None, 1, 1, 0, 1, 1, out, 1, C.byref(n), drop) == TFP_E_ARG
        assert n.value == 77 and drop[0] == 5 and out[0].hits == 9
    v = C.c_int64(3)
    assert lib.tfp_live_tracks(None, 0, None, None, None, 0, C.byref(v)) == TFP_E_ARG and v.value == 3
    assert lib.tfp_group_live_tracks(None, 0, None, None, None, 0, C.byref(v)) == TFP_E_ARG and v.value == 3
    assert lib.tfp_live_occurrence_stats(None, None, None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_live_occurrence_stats(None, 0, None, None, None, None, None) == TFP_E_ARG


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_carried_trace_equals_one_shot_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_live_trace")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_live_trace.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
