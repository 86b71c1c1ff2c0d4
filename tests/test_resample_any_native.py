"""The host arithmetic of a mixed batch (csrc/tfp_resample_any.hpp: descriptor validation, plan de-duplication up to
and past TFP_ANY_RATES_MAX, the tile counts and each clip's form at the staging constants' edges) and the kernel's own
tile routine run on the host over every tile of a batch of every class against tfp_resample_any_pcm, stand-alone under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (tests/native/check_resample_any.cpp), as the wide native
check is built. No GPU."""
import os
import subprocess

from conftest import REPO

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_any_host_arithmetic_and_tiles_asan_ubsan(tmp_path):
    exe = str(tmp_path / "check_resample_any")
    csrc = os.path.join(REPO, "asterisk-tiresias_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *ASAN, "-I" + csrc,
                    "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "native", "check_resample_any.cpp"),
                    os.path.join(csrc, "tfp_resample.cpp"), os.path.join(csrc, "tfp_wav.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
