"""Interleaved audio ingest (tfp_wav_decode_interleaved / tfp_wav_read_interleaved): 8/16-bit integer PCM of
1 to 32 channels, the samples as stored, for the multichannel rate forms. Host-only. The chunk builders are
test_wav_ingest.py's."""
import ctypes as C
import struct
import wave

import numpy as np
import pytest

from tiresias_amd import TfpError
from tiresias_amd._lib import lib
from tiresias_amd.engine import decode_wav_interleaved, read_wav_interleaved

TFP_E_CAPACITY, TFP_E_FORMAT, TFP_E_NOENT = -5, -8, -4


def chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_pcm(channels=1, rate=8000, bits=16, tag=1):
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


def test_stereo_16bit_matches_python_wave(tmp_path):
    rng = np.random.default_rng(5)
    for n, ch, sr in ((0, 2, 44100), (1, 2, 48000), (4411, 2, 44100), (1000, 1, 8000), (777, 3, 16000)):
        x = rng.integers(-32768, 32768, (n, ch), dtype=np.int16)
        path = str(tmp_path / f"c{n}_{ch}.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(x.astype("<i2").tobytes())
        got, got_sr = read_wav_interleaved(path)
        assert got_sr == sr and got.dtype == np.int16 and got.shape == (n, ch)
        with wave.open(path, "rb") as w:
            want = np.frombuffer(w.readframes(n), "<i2").reshape(n, ch)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(decode_wav_interleaved(open(path, "rb").read())[0], x)


def test_8bit_maps_exactly_onto_int16():
    u = np.arange(256, dtype=np.uint8)
    got, _ = decode_wav_interleaved(riff(fmt_pcm(channels=2, bits=8), chunk(b"data", u.tobytes())))
    assert got.shape == (128, 2)
    np.testing.assert_array_equal(got.reshape(-1).astype(np.int32), (u.astype(np.int32) - 128) * 256)


def test_extensible_six_channels_and_chunks_skipped():
    x = np.arange(-60, 60, dtype=np.int16).reshape(20, 6)
    data = riff(chunk(b"LIST", b"INFOabc"), fmt_extensible(channels=6, rate=48000), chunk(b"fact", b"\x14\0\0\0"),
                chunk(b"data", x.tobytes()), chunk(b"junk", b"zz"))
    got, sr = decode_wav_interleaved(data)
    assert sr == 48000
    np.testing.assert_array_equal(got, x)
    x32 = np.arange(64, dtype=np.int16).reshape(2, 32)
    np.testing.assert_array_equal(decode_wav_interleaved(riff(fmt_pcm(channels=32), chunk(b"data", x32.tobytes())))[0], x32)


def test_trailing_partial_frame_dropped_and_data_sizes():
    x = np.arange(30, dtype=np.int16).reshape(10, 3)
    body = x.tobytes()
    for size in (0, 0xFFFFFFFF, 1000):  # unpatched and overlong data sizes: the whole frames present
        got, _ = decode_wav_interleaved(riff(fmt_pcm(channels=3)) + b"data" + struct.pack("<I", size) + body)
        np.testing.assert_array_equal(got, x)
    for cut in (1, 2, 5):  # a partial frame at the end, truncated file and honest size alike
        got, _ = decode_wav_interleaved(riff(fmt_pcm(channels=3)) + b"data" + struct.pack("<I", 60) + body[:60 - cut])
        np.testing.assert_array_equal(got, x[:9])
        got, _ = decode_wav_interleaved(riff(fmt_pcm(channels=3), chunk(b"data", body[:60 - cut])))
        np.testing.assert_array_equal(got, x[:9])


@pytest.mark.parametrize("fmt,why", [(fmt_pcm(channels=2, bits=24), "24-bit"), (fmt_pcm(channels=2, bits=32), "32-bit"),
                                     (fmt_pcm(channels=2, tag=3, bits=32), "format tag 3"),
                                     (fmt_extensible(sub_tag=3, channels=2, bits=32), "format tag 3"),
                                     (fmt_pcm(tag=7, bits=8), "format tag 7"), (fmt_pcm(tag=6, bits=8), "format tag 6"),
                                     (fmt_pcm(channels=33), "33 channels"), (fmt_pcm(channels=0), "0 channels")])
def test_refused_with_a_reason(fmt, why):
    with pytest.raises(TfpError) as e:
        decode_wav_interleaved(riff(fmt, chunk(b"data", b"\0" * 264)))
    assert e.value.code == TFP_E_FORMAT
    assert why in lib().tfp_engine_last_error(None).decode()


def test_size_query_capacity_and_missing_file(tmp_path):
    x = np.arange(24, dtype=np.int16).reshape(12, 2)
    raw = riff(fmt_pcm(channels=2, rate=44100), chunk(b"data", x.tobytes()))
    buf = C.create_string_buffer(raw, len(raw))
    n, ch, sr = C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    assert lib().tfp_wav_decode_interleaved(buf, len(raw), None, 0, C.byref(n), C.byref(ch), C.byref(sr)) == 0
    assert (n.value, ch.value, sr.value) == (12, 2, 44100)
    out = np.full(24, 77, np.int16)
    n, ch = C.c_int64(-1), C.c_int32(-1)
    assert lib().tfp_wav_decode_interleaved(buf, len(raw), out.ctypes.data, 23, C.byref(n), C.byref(ch), None) == TFP_E_CAPACITY
    assert (n.value, ch.value) == (12, 2) and (out == 77).all()
    assert lib().tfp_wav_decode_interleaved(buf, len(raw), out.ctypes.data, 24, C.byref(n), None, None) == 0
    np.testing.assert_array_equal(out.reshape(12, 2), x)
    with pytest.raises(TfpError) as e:
        read_wav_interleaved(str(tmp_path / "missing.wav"))
    assert e.value.code == TFP_E_NOENT
