"""The device group's merge-and-keep-k of ranked search (csrc/tfp_rank_merge.hpp): host code with no
GPU call, run stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
(tests/native/check_rank_merge.cpp)."""
import os
import subprocess

from conftest import REPO

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_rank_merge_keep_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_rank_merge")
    subprocess.run(["g++", "-std=c++17", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_rank_merge.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
