"""G.711 ingest on the host: the code map (tfp_g711_decode) against the two formulas of g711_util
over all 256 codes of both laws, the WAV reader for format tags 6 and 7 (tfp_wav_decode_g711), and
a sanitizer run of both over truncated and random bytes (tests/native/g711_fuzz.cpp, a stand-alone
program). No GPU: these calls are host code."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from g711_util import ALAW, ANCHORS, ULAW, alaw_expand, chunk, expand, fmt, fmt_ext, g711_wav, riff, ulaw_expand, wav_tag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TFP_OK, TFP_E_ARG, TFP_E_CAPACITY, TFP_E_FORMAT = 0, -1, -5, -8
ALL = np.arange(256, dtype=np.uint8)


@pytest.mark.parametrize("law", [ULAW, ALAW])
def test_all_codes_equal_the_formulas(tfp_lib, law):
    got = tfp_lib.decode_g711(ALL, law)
    assert got.dtype == np.int16 and np.array_equal(got, expand(ALL, law))
    for code, value in ANCHORS[law].items():
        assert got[code] == value, (hex(code), got[code], value)


def test_ranges_and_distinct_values(tfp_lib):
    u, a = tfp_lib.decode_g711(ALL, ULAW), tfp_lib.decode_g711(ALL, ALAW)
    assert (u.min(), u.max()) == (-32124, 32124) and len(np.unique(u)) == 255  # 0x7F and 0xFF are both 0
    assert (a.min(), a.max()) == (-32256, 32256) and len(np.unique(a)) == 256
    assert np.array_equal(u, ulaw_expand(ALL)) and np.array_equal(a, alaw_expand(ALL))


@pytest.mark.parametrize("law", [ULAW, ALAW])
def test_all_codes_equal_audioop(tfp_lib, law):
    audioop = pytest.importorskip("audioop")
    lin = audioop.alaw2lin(ALL.tobytes(), 2) if law == ALAW else audioop.ulaw2lin(ALL.tobytes(), 2)
    assert np.array_equal(tfp_lib.decode_g711(ALL, law), np.frombuffer(lin, "<i2"))


def test_decode_argument_rules(tfp_lib):
    L = tfp_lib.lib()
    pcm = np.zeros(4, np.int16)
    codes = np.zeros(4, np.uint8)
    assert L.tfp_g711_decode(None, 0, ULAW, None) == TFP_OK
    assert L.tfp_g711_decode(codes.ctypes.data, 0, ALAW, pcm.ctypes.data) == TFP_OK
    for law in (-1, 2, 7):
        assert L.tfp_g711_decode(codes.ctypes.data, 4, law, pcm.ctypes.data) == TFP_E_ARG
    assert L.tfp_g711_decode(None, 4, ULAW, pcm.ctypes.data) == TFP_E_ARG
    assert L.tfp_g711_decode(codes.ctypes.data, 4, ULAW, None) == TFP_E_ARG
    assert L.tfp_g711_decode(codes.ctypes.data, -1, ULAW, pcm.ctypes.data) == TFP_E_ARG


@pytest.mark.parametrize("rate", [8000, 16000])
@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("law", [ULAW, ALAW])
def test_wav_round_trip(tfp_lib, law, extensible, rate):
    codes = np.concatenate([ALL, ALL[::-1]])
    got, sr, got_law = tfp_lib.decode_wav_g711(g711_wav(codes, law, rate, extensible))
    assert np.array_equal(got, codes) and sr == rate and got_law == law


def test_wav_read_from_a_file(tfp_lib, tmp_path):
    path = tmp_path / "prompt.wav"
    path.write_bytes(g711_wav(ALL, ALAW))
    got, sr, law = tfp_lib.read_wav_g711(str(path))
    assert np.array_equal(got, ALL) and (sr, law) == (8000, ALAW)
    with pytest.raises(tfp_lib.TfpError) as e:
        tfp_lib.read_wav_g711(str(tmp_path / "missing.wav"))
    assert e.value.code == -4


@pytest.mark.parametrize("law", [ULAW, ALAW])
def test_wav_odd_size_pad_and_following_chunk(tfp_lib, law):
    codes = ALL[:255]  # odd: a pad byte follows, then another chunk that is not audio
    raw = riff(fmt(wav_tag(law)), chunk(b"data", codes.tobytes()), chunk(b"LIST", b"INFOxxxx"))
    got, _, got_law = tfp_lib.decode_wav_g711(raw)
    assert np.array_equal(got, codes) and got_law == law


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_wav_unpatched_size_takes_what_is_there(tfp_lib, size):
    body = ALL[:201].tobytes()
    raw = riff(fmt(7)) + b"data" + struct.pack("<I", size) + body
    got, _, law = tfp_lib.decode_wav_g711(raw)
    assert np.array_equal(got, ALL[:201]) and law == ULAW


def test_wav_truncated_data(tfp_lib):
    raw = riff(fmt(6)) + b"data" + struct.pack("<I", 100) + ALL[:37].tobytes()
    got, _, law = tfp_lib.decode_wav_g711(raw)
    assert np.array_equal(got, ALL[:37]) and law == ALAW


def test_wav_size_query_and_capacity(tfp_lib):
    L = tfp_lib.lib()
    raw = g711_wav(ALL, ULAW, 16000)
    buf = C.create_string_buffer(raw, len(raw))
    n, sr, law = C.c_int64(-1), C.c_int32(), C.c_int32(-1)
    assert L.tfp_wav_decode_g711(buf, len(raw), None, 0, C.byref(n), C.byref(sr), C.byref(law)) == TFP_OK
    assert (n.value, sr.value, law.value) == (256, 16000, ULAW)
    small = np.full(300, 0xEE, np.uint8)
    n2 = C.c_int64(-1)
    assert L.tfp_wav_decode_g711(buf, len(raw), small.ctypes.data, 255, C.byref(n2), None, None) == TFP_E_CAPACITY
    assert n2.value == 256 and (small == 0xEE).all()
    assert "255 of 256" in L.tfp_engine_last_error(None).decode()
    assert L.tfp_wav_decode_g711(buf, len(raw), small.ctypes.data, 300, C.byref(n2), None, None) == TFP_OK
    assert np.array_equal(small[:256], ALL) and (small[256:] == 0xEE).all()
    assert L.tfp_wav_decode_g711(None, 0, None, 0, C.byref(n2), None, None) == TFP_E_ARG
    assert L.tfp_wav_decode_g711(buf, len(raw), None, 0, None, None, None) == TFP_E_ARG
    assert L.tfp_wav_decode_g711(buf, len(raw), None, 4, C.byref(n2), None, None) == TFP_E_ARG


REFUSALS = [
    ("tag 1", riff(fmt(1, bits=16), chunk(b"data", b"\0" * 32)), "format tag 1"),
    ("tag 3", riff(fmt(3, bits=32), chunk(b"data", b"\0" * 32)), "format tag 3"),
    ("extensible pcm", riff(fmt_ext(1, bits=16), chunk(b"data", b"\0" * 32)), "format tag 1"),
    ("2 channels", riff(fmt(7, channels=2), chunk(b"data", b"\0" * 32)), "2 channels"),
    ("16 bits", riff(fmt(6, bits=16), chunk(b"data", b"\0" * 32)), "16-bit"),
    ("block align", riff(fmt(7, align=2), chunk(b"data", b"\0" * 32)), "block align"),
    ("not riff", b"RIFX" + b"\0" * 40, "RIFF/WAVE"),
    ("no data", riff(fmt(7)), "no data chunk"),
]


@pytest.mark.parametrize("name,raw,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_wav_refusals_carry_a_reason(tfp_lib, name, raw, reason):
    with pytest.raises(tfp_lib.TfpError) as e:
        tfp_lib.decode_wav_g711(raw)
    assert e.value.code == TFP_E_FORMAT and reason in str(e.value), str(e.value)


@pytest.mark.parametrize("law", [ULAW, ALAW])
def test_pcm_decoders_keep_refusing_g711(tfp_lib, law):
    from tiresias_amd.engine import decode_wav, decode_wav_f32
    raw = g711_wav(ALL, law)
    for dec in (decode_wav, decode_wav_f32):
        with pytest.raises(tfp_lib.TfpError) as e:
            dec(raw)
        assert e.value.code == TFP_E_FORMAT


def test_fuzz_under_sanitizers(tmp_path):
    """tests/native/g711_fuzz.cpp with csrc/tfp_wav.cpp, AddressSanitizer + UBSan, run as a child."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "g711_fuzz"
    csrc = os.path.join(REPO, "asterisk-tiresias_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"), "-I", csrc,
                    os.path.join(REPO, "tests", "native", "g711_fuzz.cpp"), os.path.join(csrc, "tfp_wav.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("g711_fuzz ok"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
