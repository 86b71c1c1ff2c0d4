"""Catalog neighbours, host side (csrc/tfp_neighbour.hpp), stand-alone under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU (tests/native/check_neighbour.cpp): the row-to-frame-value map
tfp::neighbour_frame_value, the one the kernels call frame_key and frame_box on (no integer key form exists,
so none is pinned), against Python's parse of the "%f" text the reference stored; the "k + 1 rows minus self"
routine and the device group's merge. No GPU."""
import os
import random
import subprocess

import pytest

from conftest import REPO

INT32_MAX, INT32_MIN = 2**31 - 1, -(2**31)
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("neighbour") / "check_neighbour")
    subprocess.run(["g++", "-std=c++17", *ASAN, "-I" + os.path.join(REPO, "asterisk-tiresias_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "check_neighbour.cpp"), "-o", out], check=True)
    return out


def _text(m: int) -> str:
    """The "%f" text of the stored value m micro-units: sign, integer part, six decimals."""
    a = abs(m)
    return "%s%d.%06d" % ("-" if m < 0 else "", a // 10**6, a % 10**6)


def _inputs():
    ms = [INT32_MAX, INT32_MIN + 1]
    for ip in range(-120, 121):
        for frac in (0, 1, 999999):
            for sign in (1, -1):
                ms.append(ip * 10**6 + sign * frac)
    rng = random.Random(20240611)
    ms += [rng.randint(INT32_MIN + 1, INT32_MAX) for _ in range(100000)]
    return ms


def test_row_to_frame_value_is_the_text_parse(exe):
    """The native map on every input against float() of the decimal text, and (int) of it against the
    decimal's truncation; a stored NULL is -inf."""
    assert _text(12345678) == "12.345678" and _text(-1) == "-0.000001" and _text(INT32_MAX) == "2147.483647"
    ms = _inputs()
    r = subprocess.run([exe, "--map"], input="\n".join(map(str, ms + [INT32_MIN])) + "\n", capture_output=True, text=True,
                       timeout=300, env=SAN_ENV)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = [float.fromhex(x) for x in r.stdout.split()]
    assert len(got) == len(ms) + 1 and got[-1] == float("-inf")
    bad = [m for m, v in zip(ms, got) if v != float(_text(m)) or int(v) != (abs(m) // 10**6) * (1 if m >= 0 else -1)]
    assert not bad, bad[:10]


def test_drop_self_and_group_merge_asan_ubsan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=SAN_ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
