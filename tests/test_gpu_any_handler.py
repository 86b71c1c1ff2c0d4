"""The mirror's directory enrolment with mixed_batch: a directory of six files of different rates, channel counts
and sample kinds (and one at the index rate) enrolled by FpHandler(index_rate=8000, mix_channels=True,
wide_samples=True, mixed_batch=True) through ONE fingerprint_any_batch gives the catalog rows, the stored
fingerprints and the search results of the same handler with mixed_batch=False, which makes one call per group and
no mixed launch."""
import struct
import wave

import numpy as np
import pytest

from resample_util import class_clip

pytestmark = pytest.mark.gpu


def _write_wav(path, x, rate, width=2):
    x = np.asarray(x)
    x = x.reshape(len(x), -1)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        if width == 2:
            w.writeframes(x.astype("<i2").tobytes())
        elif width == 3:  # the int16 value in the upper two bytes, noise below
            lo = np.random.default_rng(len(x)).integers(0, 256, x.shape)
            w.writeframes(((x.astype("<i4") << 8) + lo).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes())
        else:
            lo = np.random.default_rng(len(x)).integers(0, 65536, x.shape)
            w.writeframes(((x.astype("<i4") << 16) + lo).astype("<i4").tobytes())


def _write_g711_wav(path, codes, rate, tag):
    """A mono G.711 WAV: format tag 7 (mu-law) or 6 (A-law), 8 bits per sample."""
    codes = np.ascontiguousarray(codes, np.uint8)
    fmt = struct.pack("<HHIIHHH", tag, 1, rate, rate, 1, 8, 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(codes)) + codes.tobytes()
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body + (b"\0" if len(codes) % 2 else b""))


def _stereo(x, seed):
    side = np.random.default_rng(seed).integers(-200, 201, len(x))
    return np.clip(np.stack([x.astype(np.int32) + side, x.astype(np.int32) - side], 1), -32768, 32767).astype(np.int16)


def _ulaw_codes(tfp_lib, x):
    """The mu-law code whose expansion is nearest each sample (a search over the 256 expansions)."""
    table = tfp_lib.decode_g711(np.arange(256, dtype=np.uint8), tfp_lib.ULAW).astype(np.int32)
    return np.abs(x.astype(np.int32)[:, None] - table[None, :]).argmin(1).astype(np.uint8)


def _enrol(tfp_lib, d, mixed, monkeypatch):
    from tiresias_amd import FpHandler
    # the same uuids in both handlers: ties between clips are broken by uuid, and the two runs are compared row for row
    ids = iter("%08x-a11c-4000-8000-%012x" % (i * 2654435761 % 2**32, i) for i in range(100))
    monkeypatch.setattr(FpHandler, "fp_generate_uuid", staticmethod(lambda: next(ids)))
    h = FpHandler(0, index_rate=8000, mix_channels=True, wide_samples=True, mixed_batch=mixed)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        a0 = h.engine.resample_any_stats()
        assert h.create_new_audio_info("ctx"), h.last_error
        a1 = h.engine.resample_any_stats()
        rows = h.fp_get_audio_lists_all()
        stored = {r["name"]: h.engine.index_rows(r["uuid"]) for r in rows}
        names = {r["uuid"]: r["name"] for r in rows}
        found = {}
        for r in rows:
            got = h.fp_search_fingerprint_info("ctx", str(d / r["name"]), 1, 0.45, -1, -1)
            found[r["name"]] = None if got is None else (names[got["uuid"]], got["match_count"], got["frame_count"])
        return [(r["uuid"], r["name"], r["context"], r["hash"]) for r in rows], stored, found, a1["launches"] - a0["launches"], a1["clips"] - a0["clips"]
    finally:
        h.fp_term()


def test_mixed_enrolment_equals_the_per_group_enrolment(tfp_lib, tmp_path, monkeypatch):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    d = tmp_path / "prompts"
    d.mkdir()
    src = [class_clip(k, 16000) for k in (0, 1, 2)] + list(tfp_lib.synth_pcm(0x7153A1, range(4), 16000))
    up = lambda x, r: tfp_lib.resample_pcm(x, 8000, r)  # noqa: E731
    _write_wav(d / "a_16k_mono16.wav", up(src[0], 16000), 16000)
    _write_wav(d / "b_44k_stereo16.wav", _stereo(up(src[1], 44100), 1), 44100)
    _write_wav(d / "c_48k_stereo24.wav", _stereo(up(src[2], 48000), 2), 48000, width=3)
    _write_wav(d / "d_44k_mono32.wav", up(src[3], 44100), 44100, width=4)
    _write_g711_wav(d / "e_16k_ulaw.wav", _ulaw_codes(tfp_lib, up(src[4], 16000)), 16000, 7)
    _write_wav(d / "f_16k_stereo16.wav", _stereo(up(src[5], 16000), 3), 16000)
    _write_wav(d / "g_8k_mono16.wav", src[6], 8000)  # at the index rate: its own path either way
    rows1, stored1, found1, launches1, clips1 = _enrol(tfp_lib, d, True, monkeypatch)
    rows0, stored0, found0, launches0, _ = _enrol(tfp_lib, d, False, monkeypatch)
    assert launches1 == 1 and clips1 == 6 and launches0 == 0
    assert [r[1] for r in rows1] == sorted(r[1] for r in rows1) and len(rows1) == 7
    assert rows1 == rows0
    for name in stored0:
        assert len(stored0[name][0]) > 0
        assert np.array_equal(stored1[name][0], stored0[name][0]) and np.array_equal(stored1[name][1], stored0[name][1]), name
    assert found1 == found0
    # the searches are not vacuous: each of these files finds an enrolled clip
    assert all(found1[n] is not None and found1[n][1] > 0 for n in ("a_16k_mono16.wav", "b_44k_stereo16.wav", "c_48k_stereo24.wav"))
