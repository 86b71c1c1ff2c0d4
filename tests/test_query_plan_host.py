"""A search batch's offset arithmetic (csrc/tfp_query_plan.hpp: the monotone check, relative and sample
offsets to frame offsets, the sliding forms' window offsets and capacity verdict, the census's bins): no GPU
call, run stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
(tests/native/check_query_plan.cpp); the counts it prints are compared with the library's exported
tfp_frame_count and tfp_sliding_windows."""
import os
import subprocess

from conftest import REPO

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_query_plan_header_asan_ubsan(tmp_path, tfp_lib):
    exe = str(tmp_path / "check_query_plan")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_query_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
    # the header's frame and window counts are the ones the library exports
    lines = [ln.split() for ln in r.stdout.splitlines()]
    frames = [tuple(map(int, ln[1:])) for ln in lines if ln[0] == "frames"]
    windows = [tuple(map(int, ln[1:])) for ln in lines if ln[0] == "windows"]
    assert len(frames) == 5 and len(windows) == 6
    assert all(tfp_lib.frame_count(n) == f for n, f in frames)
    assert all(tfp_lib.sliding_windows(n, w, h) == got for n, w, h, got in windows)
