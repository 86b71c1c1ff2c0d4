"""csrc/tfp_math.hpp micro_of_coef_fast (the throughput kernel's fused tail finish) vs this host's glibc.

Wherever the fast finish decides, its micro-units equal micro_of_db(10.0 * log10(fabs((double)c))); with
the slow path where it does not, they are equal for every float. Sampled here (a strided walk of all
2^32 bit patterns, the special inputs, the neighbours of 1.0 and the floats nearest a half-micro
boundary, tests/golden/micro_fast_boundary.txt); the exhaustive run's log is
profiles/r07/check_micro_fast_exhaustive.txt."""
import os
import re
import subprocess

from conftest import REPO

NATIVE = os.path.join(REPO, "tests", "native")
BOUNDARY = os.path.join(REPO, "tests", "golden", "micro_fast_boundary.txt")


def test_micro_fast_sampled(tmp_path):
    exe = str(tmp_path / "check_micro_fast")
    subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-fno-builtin", "-fopenmp",
                    os.path.join(NATIVE, "check_micro_fast.cpp"), "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe, "997", BOUNDARY], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout
    assert "decided but != glibc : 0\n" in out.stdout
    assert "with the slow path where undecided, != glibc : 0\n" in out.stdout
    assert "zeros/inf/NaN undecided : 0\n" in out.stdout
    m = re.search(r"listed patterns: (\d+), decided but != glibc : 0, combined != glibc : 0, undecided : (\d+)", out.stdout)
    # the list: 24 specials, 258 around 1.0, 768 bucket ends, the 64 boundary floats (all undecided,
    # as the 6 subnormals are)
    assert m and int(m.group(1)) == 24 + 258 + 768 + 64 and int(m.group(2)) >= 64 + 6, out.stdout


def test_micro_fast_exhaustive_log_committed():
    log = open(os.path.join(REPO, "profiles", "r07", "check_micro_fast_exhaustive.txt")).read()
    assert "stride 1: 4294967296 patterns (4278190078 finite non-zero)" in log
    assert "decided but != glibc : 0\n" in log
    assert "with the slow path where undecided, != glibc : 0\n" in log
    assert log.strip().endswith("OK")
    near = re.findall(r"^near (0x[0-9a-f]{8}) ", log, re.M)
    assert near == open(BOUNDARY).read().split()
