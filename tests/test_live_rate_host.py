"""The host arithmetic of a live object with an input rate (csrc/tfp_live_rate.hpp): the settled count, the
carry bound, the streaming routine against the whole-clip map under random splits, the zero flush, the
tile table and the capacity refusal, run stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer
on the CPU (tests/native/check_live_rate.cpp). No GPU."""
import os
import subprocess

from conftest import REPO

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_live_rate_arithmetic_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_live_rate")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_live_rate.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
