"""Q31 audio ingest (tfp_wav_decode_interleaved_q31 / tfp_wav_read_interleaved_q31): integer PCM of 8, 16, 24
or 32 bits and float of 32 or 64 bits, format 1, format 3 and EXTENSIBLE, 1 to 32 channels, each sample as
int32 Q31, for the wide rate forms. Host-only. The WAVs are built with struct."""
import ctypes as C
import struct

import numpy as np
import pytest

from tiresias_amd import TfpError, q31_from_float
from tiresias_amd._lib import lib
from tiresias_amd.engine import decode_wav_interleaved_q31, read_wav_interleaved_q31

TFP_E_CAPACITY, TFP_E_FORMAT, TFP_E_NOENT = -5, -8, -4


def chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_plain(channels=1, rate=8000, bits=16, tag=1):
    align = channels * bits // 8
    return chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits))


def fmt_extensible(sub_tag=1, channels=1, rate=8000, bits=16):
    align = channels * bits // 8
    guid = struct.pack("<H", sub_tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    body = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits, 4) + guid
    return chunk(b"fmt ", body)


def riff(*chunks: bytes) -> bytes:
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def encode(kind, n, ch, seed):
    """(data bytes, expected int32 Q31 [n, ch]) of random samples with the extremes in front, for one stored kind."""
    rng = np.random.default_rng(seed)
    total = n * ch
    if kind == "u8":
        u = rng.integers(0, 256, total).astype(np.uint8)
        u[:2] = (0, 255)
        return u.tobytes(), ((u.astype(np.int64) - 128) << 24).astype(np.int32).reshape(n, ch)
    if kind == "i16":
        x = rng.integers(-2**15, 2**15, total).astype("<i2")
        x[:2] = (-2**15, 2**15 - 1)
        return x.tobytes(), (x.astype(np.int32) << 16).reshape(n, ch)
    if kind == "i24":
        x = rng.integers(-2**23, 2**23, total).astype(np.int32)
        x[:2] = (-2**23, 2**23 - 1)
        raw = b"".join(struct.pack("<i", int(v))[:3] for v in x)
        return raw, (x << 8).reshape(n, ch)
    if kind == "i32":
        x = rng.integers(-2**31, 2**31, total).astype("<i4")
        x[:2] = (-2**31, 2**31 - 1)
        return x.tobytes(), x.astype(np.int32).reshape(n, ch)
    x = rng.standard_normal(total) * 0.4
    x[:6] = (1.0, -1.0, 1.5, float("nan"), float("inf"), 3 * 2.0**-32)
    x = x.astype("<f4" if kind == "f32" else "<f8")
    return x.tobytes(), q31_from_float(x).reshape(n, ch)  # (the float maps have their own test, test_resample_wide_host.py)


KINDS = {"u8": (1, 8), "i16": (1, 16), "i24": (1, 24), "i32": (1, 32), "f32": (3, 32), "f64": (3, 64)}


@pytest.mark.parametrize("ch", [1, 2, 32])
@pytest.mark.parametrize("extensible", [False, True], ids=["plain", "extensible"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_width_and_format_tag(tmp_path, kind, extensible, ch):
    tag, bits = KINDS[kind]
    n = 40
    raw, want = encode(kind, n, ch, 11 * ch + bits)
    fmt = fmt_extensible(tag, ch, 48000, bits) if extensible else fmt_plain(ch, 48000, bits, tag)
    data = riff(chunk(b"LIST", b"INFOabc"), fmt, chunk(b"fact", b"\x28\0\0\0"), chunk(b"data", raw), chunk(b"junk", b"zz"))
    got, sr = decode_wav_interleaved_q31(data)
    assert sr == 48000 and got.dtype == np.int32 and got.shape == (n, ch)
    np.testing.assert_array_equal(got, want)
    path = tmp_path / "x.wav"
    path.write_bytes(data)
    got2, sr2 = read_wav_interleaved_q31(str(path))
    assert sr2 == 48000
    np.testing.assert_array_equal(got2, want)


def test_float_extremes_in_a_file():
    x = np.array([1.0, -1.0, 1.5, -7.0, np.nan, np.inf, -np.inf, 0.5, 2.0**-32, 3 * 2.0**-32, 0.0, -0.0])
    want = [2**31 - 1, -2**31, 2**31 - 1, -2**31, 0, 2**31 - 1, -2**31, 2**30, 0, 2, 0, 0]
    for dt, bits in (("<f4", 32), ("<f8", 64)):
        got, _ = decode_wav_interleaved_q31(riff(fmt_plain(2, 44100, bits, 3), chunk(b"data", x.astype(dt).tobytes())))
        assert got.reshape(-1).tolist() == want


@pytest.mark.parametrize("kind", ["i24", "f32"])
def test_trailing_partial_frame_dropped_and_data_sizes(kind):
    tag, bits = KINDS[kind]
    raw, want = encode(kind, 10, 3, 5)
    w = bits // 8 * 3
    head = riff(fmt_plain(3, 44100, bits, tag))
    for size in (0, 0xFFFFFFFF, 100000):  # unpatched and overlong data sizes: the whole frames present
        got, _ = decode_wav_interleaved_q31(head + b"data" + struct.pack("<I", size) + raw)
        np.testing.assert_array_equal(got, want)
    for cut in (1, w // 2, w - 1):  # a partial frame at the end, truncated file and honest size alike
        got, _ = decode_wav_interleaved_q31(head + b"data" + struct.pack("<I", len(raw)) + raw[:len(raw) - cut])
        np.testing.assert_array_equal(got, want[:9])
        got, _ = decode_wav_interleaved_q31(riff(fmt_plain(3, 44100, bits, tag), chunk(b"data", raw[:len(raw) - cut])))
        np.testing.assert_array_equal(got, want[:9])


@pytest.mark.parametrize("fmt,why", [(fmt_plain(tag=7, bits=8), "format tag 7"), (fmt_plain(tag=6, bits=8), "format tag 6"),
                                     (fmt_extensible(sub_tag=7, bits=8), "format tag 7"),
                                     (fmt_plain(channels=33, bits=24), "33 channels"), (fmt_plain(channels=0, bits=32), "0 channels"),
                                     (fmt_plain(tag=3, bits=16), "16-bit"), (fmt_plain(tag=1, bits=64), "64-bit"),
                                     (fmt_plain(tag=1, bits=12), "12-bit"), (fmt_plain(tag=85, bits=16), "format tag 85")])
def test_refused_with_a_reason(fmt, why):
    with pytest.raises(TfpError) as e:
        decode_wav_interleaved_q31(riff(fmt, chunk(b"data", b"\0" * 264)))
    assert e.value.code == TFP_E_FORMAT
    assert why in lib().tfp_engine_last_error(None).decode()


def test_bad_block_align_and_missing_chunks():
    bad = chunk(b"fmt ", struct.pack("<HHIIHH", 1, 2, 44100, 44100 * 6, 5, 24))
    for data, why in ((riff(bad, chunk(b"data", b"\0" * 60)), "block align"), (riff(fmt_plain(2, 44100, 24)), "no data chunk"),
                      (riff(chunk(b"data", b"\0" * 60)), "data chunk before fmt"), (b"RIFX" + b"\0" * 40, "not a RIFF/WAVE")):
        with pytest.raises(TfpError) as e:
            decode_wav_interleaved_q31(data)
        assert e.value.code == TFP_E_FORMAT and why in lib().tfp_engine_last_error(None).decode()


def test_size_query_capacity_and_missing_file(tmp_path):
    raw, want = encode("i24", 12, 2, 9)
    data = riff(fmt_plain(2, 44100, 24), chunk(b"data", raw))
    buf = C.create_string_buffer(data, len(data))
    n, ch, sr = C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    assert lib().tfp_wav_decode_interleaved_q31(buf, len(data), None, 0, C.byref(n), C.byref(ch), C.byref(sr)) == 0
    assert (n.value, ch.value, sr.value) == (12, 2, 44100)
    out = np.full(24, 77, np.int32)
    n, ch = C.c_int64(-1), C.c_int32(-1)
    assert lib().tfp_wav_decode_interleaved_q31(buf, len(data), out.ctypes.data, 23, C.byref(n), C.byref(ch), None) == TFP_E_CAPACITY
    assert (n.value, ch.value) == (12, 2) and (out == 77).all()
    assert lib().tfp_wav_decode_interleaved_q31(buf, len(data), out.ctypes.data, 24, C.byref(n), None, None) == 0
    np.testing.assert_array_equal(out.reshape(12, 2), want)
    assert lib().tfp_wav_decode_interleaved_q31(None, 0, None, 0, C.byref(n), None, None) == -1
    with pytest.raises(TfpError) as e:
        read_wav_interleaved_q31(str(tmp_path / "missing.wav"))
    assert e.value.code == TFP_E_NOENT
