"""The wide (int32 Q31) routines of csrc/tfp_resample.hpp at their edges against an independent __int128 sum,
and the kernel's staging arithmetic run on the host against the whole-clip routine for every tile of a 2-tile
clip, stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
(tests/native/check_resample_wide.cpp), as the mix native check is built. No GPU."""
import os
import subprocess

from conftest import REPO

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_wide_routines_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_resample_wide")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_resample_wide.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
