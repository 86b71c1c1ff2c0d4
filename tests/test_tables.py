"""The product's host-built DSP tables (csrc/tfp_tables.cpp) equal the oracle's, bit for bit, and
the schedules the kernels read rebuild the dense filterbank at every sample-rate class."""
import os
import re
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import REPO

NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "asterisk-tiresias_amd", "csrc")
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin"]

# One rate per shape of tables build_tables makes (check_slot_schedule prints the shape):
# rate -> (ms_len, ms_total, ms_maxbin, ms_c_defer, empty filters, one-bin filters, fb_ok)
CLASS_SHAPES = {
    1: ((0, 0, 0), 0, 257, 1, 40, 0, 0),           # every filter empty
    100: ((0, 0, 0), 0, 257, 1, 40, 0, 0),
    500: ((120, 0, 0), 1920, 324, 1, 38, 0, 0),    # ms_total > 960: the kernel's weights stay in global memory
    1000: ((72, 0, 0), 1152, 308, 1, 34, 0, 0),
    2000: ((40, 0, 0), 640, 276, 1, 27, 0, 0),     # slots 1 and 2 of length 0
    3000: ((36, 24, 0), 960, 264, 1, 21, 0, 0),    # deferral on with no real filter in slot 2
    4000: ((36, 20, 0), 896, 272, 1, 16, 1, 0),
    6000: ((32, 16, 0), 768, 272, 1, 11, 0, 0),
    7999: ((36, 16, 8), 960, 272, 1, 6, 0, 1),     # the 8 kHz shape on other weights
    8000: ((36, 16, 8), 960, 272, 1, 6, 0, 1),
    8001: ((36, 16, 8), 960, 272, 1, 6, 0, 1),
    11025: ((36, 16, 8), 960, 276, 0, 2, 0, 0),    # the 8 kHz slot lengths with deferral off
    12000: ((36, 16, 8), 960, 272, 0, 0, 1, 0),
    16000: ((32, 12, 8), 832, 257, 0, 0, 0, 0),
    22050: ((24, 12, 8), 704, 257, 0, 0, 0, 0),
    24000: ((24, 8, 4), 576, 257, 0, 0, 0, 0),
    32000: ((16, 8, 4), 448, 257, 0, 0, 0, 0),
    44100: ((12, 8, 4), 384, 257, 0, 0, 6, 0),
    48000: ((12, 8, 4), 384, 257, 0, 0, 8, 0),
    88200: ((8, 4, 4), 256, 257, 0, 0, 21, 0),
    96000: ((8, 4, 4), 256, 257, 0, 0, 24, 0),
    192000: ((8, 4, 4), 256, 257, 0, 0, 33, 0),
    1000000: ((4, 4, 4), 192, 257, 0, 0, 40, 0),   # every filter one bin wide
}
AUDIO_RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000]
assert set(AUDIO_RATES) <= set(CLASS_SHAPES)


def _compile(tmp, name, *extra):
    exe = str(tmp / name)
    subprocess.run(GXX + ["-I", CSRC, os.path.join(NATIVE, name + ".cpp"), os.path.join(CSRC, "tfp_tables.cpp"), "-o", exe,
                          *extra], check=True)
    return exe


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("dump"), "dump_tables")


@pytest.fixture(scope="module")
def slot_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("slot"), "check_slot_schedule")


@pytest.mark.parametrize("sr", [8000, 16000, 44100] + [r for r in CLASS_SHAPES if r not in (8000, 16000, 44100)])
def test_product_tables_equal_oracle(oracle, dump_exe, tmp_path, sr):
    """Every class rate and every audio rate: the oracle's tfo_build_tables and the product's
    build_tables both accept it (neither refuses a positive rate the other takes: aubio 0.4.5's
    aubio_filterbank_set_triangle_bands only warns when bands pass Nyquist and goes on), and the
    window, twiddles, DCT and dense filterbank are equal bit for bit."""
    out = str(tmp_path / "t.bin")
    r = subprocess.run([dump_exe, str(sr), out], capture_output=True, text=True)
    assert r.returncode == 0, (sr, r.stdout, r.stderr)  # the product accepts the rate
    sizes = r.stdout.split()
    raw = open(out, "rb").read()
    nt = int(sizes[0])
    f = np.frombuffer(raw[:nt], np.uint8)
    window = np.frombuffer(f[:2048].tobytes(), np.float32)
    o = 2048
    tw256_re = np.frombuffer(f[o:o + 1024].tobytes(), np.float32); o += 1024
    tw256_im = np.frombuffer(f[o:o + 1024].tobytes(), np.float32); o += 1024
    tw512_re = np.frombuffer(f[o:o + 1028].tobytes(), np.float32); o += 1028
    tw512_im = np.frombuffer(f[o:o + 1028].tobytes(), np.float32); o += 1028
    dct = np.frombuffer(f[o:o + 320].tobytes(), np.float32).reshape(2, 40)
    mel = np.frombuffer(raw[nt:], np.float32).reshape(40, 257)

    t = oracle.tables(sr)  # raises if the oracle refuses the rate
    as_ = lambda a: np.ctypeslib.as_array(a).view(np.uint32)
    assert np.array_equal(window.view(np.uint32), as_(t.window))
    assert np.array_equal(tw256_re.view(np.uint32), as_(t.tw256_re))
    assert np.array_equal(tw256_im.view(np.uint32), as_(t.tw256_im))
    assert np.array_equal(tw512_re.view(np.uint32), as_(t.tw512_re))
    assert np.array_equal(tw512_im.view(np.uint32), as_(t.tw512_im))
    assert np.array_equal(dct.view(np.uint32), np.ctypeslib.as_array(t.dct).reshape(2, 40).view(np.uint32))
    assert np.array_equal(mel.view(np.uint32), np.ctypeslib.as_array(t.mel).reshape(40, 257).view(np.uint32))
    empty = int((~mel.view(np.uint32).any(axis=1)).sum())
    assert empty == CLASS_SHAPES[sr][4]  # the oracle's own dense rows have the class's empty filters


def test_tables_refuse_only_rates_below_one(oracle, dump_exe, tmp_path):
    """Both sides refuse the rates <= 0 (the product's other refusal, ms_maxbin > 500, is met by no
    rate: test_slot_schedule_sweep) and take the least and a huge positive one."""
    for sr in (0, -8000):
        with pytest.raises(ValueError):
            oracle.tables(sr)
        assert subprocess.run([dump_exe, str(sr), str(tmp_path / "t.bin")], capture_output=True).returncode == 1
    for sr in (1, 2**31 - 1):
        oracle.tables(sr)
        assert subprocess.run([dump_exe, str(sr), str(tmp_path / "t.bin")], capture_output=True).returncode == 0


def test_frame_pair_schedule_8k(tmp_path):
    """The throughput kernel's frame-pair filterbank schedule (csrc/tfp_tables.cpp
    build_fb_schedule) rebuilds every 8 kHz filter's dense row bit for bit, one job per filter."""
    exe = _compile(tmp_path, "check_fb_schedule")
    r = subprocess.run([exe, "8000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK: 34 filters")
    r = subprocess.run([exe, "16000"], capture_output=True, text=True)  # the rate argument is honoured
    assert r.returncode == 3 and "no frame-pair schedule at 16000 Hz" in r.stdout


SHAPE_RE = re.compile(r"rate (\d+) len (\d+) (\d+) (\d+) total (\d+) maxbin (\d+) defer (\d) real (-?\d+) (-?\d+) "
                      r"empty (\d+) onebin (\d+) fb (\d) nf (-?\d+)$")


def test_slot_schedule_class_rates(slot_exe):
    """check_slot_schedule at one rate per class of tables and at the audio rates: the sparse
    filters, the slot schedule as the kernels index it, the deferral flags and the frame-pair
    schedule rebuild the dense filterbank bit for bit, and each rate has the shape its class is
    named for (which the GPU tests of these rates rely on)."""
    r = subprocess.run([slot_exe] + [str(sr) for sr in CLASS_SHAPES], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("OK: %d rates, 0 rejected" % len(CLASS_SHAPES)), lines[-1]
    got = {}
    for ln in lines[:-1]:
        m = SHAPE_RE.match(ln)
        assert m, ln
        v = [int(x) for x in m.groups()]
        got[v[0]] = ((v[1], v[2], v[3]), v[4], v[5], v[6], v[9], v[10], v[11])
        if v[11]:
            assert v[12] == 40 - v[9]  # fb_nfilters taken from the tables
        if v[6] and v[3] == 0:
            assert (v[7], v[8]) == (-1, -1)
    assert got == CLASS_SHAPES


def test_slot_schedule_sweep(slot_exe):
    """The same checks at every rate from 1 to 2,000, at every 499th rate from there to 400,000, and
    at every rate around 8,000 whose tables take the 8 kHz kernels. build_tables refuses none of
    them: its ms_maxbin > 500 branch is not reachable (a slot's longest span is a filter at least
    133 Hz wide cut off at Nyquist, at most ~130 bins, read from a bin <= 256).

    Measured: 1.2 s on 8 cores (9 s of CPU time, nearly all of it the lane-order searches of
    lane_order_for_banks and, near 8 kHz, fb_order_for_banks), the greatest ms_maxbin 384."""
    n = max(1, min(8, os.cpu_count() or 1))
    stride = 499
    jobs = [["%d:2000:%d" % (1 + k, n), "%d:400000:%d" % (2001 + k * stride, n * stride)] for k in range(n)]
    jobs.append(["7940:8040:1"])
    t0 = time.time()
    with ThreadPoolExecutor(len(jobs)) as ex:
        res = list(ex.map(lambda a: subprocess.run([slot_exe] + a, capture_output=True, text=True), jobs))
    print("sweep: %.2f s on %d workers" % (time.time() - t0, n))
    nrates, maxbin = 0, 0
    for r in res:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        m = re.match(r"OK: (\d+) rates, (\d+) rejected, ms_maxbin <= (\d+)$", r.stdout.strip().splitlines()[-1])
        assert m and int(m.group(2)) == 0, r.stdout[-2000:]
        assert "rejected\n" not in r.stdout
        nrates += int(m.group(1))
        maxbin = max(maxbin, int(m.group(3)))
    assert nrates == 2000 + len(range(2001, 400001, stride)) + 101
    assert 257 <= maxbin <= 500
    print("greatest ms_maxbin:", maxbin)
    # the rates around 8 kHz whose tables have the 8 kHz shape (they run the 8 kHz kernels)
    runs = re.findall(r"fixedshape (\d+)-(\d+)", res[-1].stdout)
    assert any(int(a) <= 7999 and 8001 <= int(b) for a, b in runs), runs
    print("8 kHz-shaped tables at:", runs)
