"""The fp_handler mirror with wide_samples: a 24-bit stereo 48 kHz WAV and a float32 mono 44.1 kHz WAV are enrolled
at the index's rate through the Q31 reader and the wide form (one launch per (channels, rate) group), and each is
found by a search with the same audio at 8 kHz int16 as the host converter gives it; a file search and a single
file's enrolment convert on the host; the same handler without wide_samples refuses both files with the message
it had before the option."""
import struct

import numpy as np
import pytest

from resample_util import class_clip

pytestmark = pytest.mark.gpu


def _chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _write(path, tag, bits, rate, channels, data):
    align = channels * bits // 8
    fmt = _chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits))
    body = b"WAVE" + fmt + _chunk(b"data", data)
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


def _pcm24_stereo(tfp_lib, clip, seed):
    """The clip at 48 kHz on two 24-bit channels (plus and minus a difference signal, the low byte filled)."""
    up = tfp_lib.resample_pcm(clip, 8000, 48000).astype(np.int64) << 8
    rng = np.random.default_rng(seed)
    side = rng.integers(-200 << 8, (200 << 8) + 1, len(up))
    x = np.clip(np.stack([up + side, up - side], 1) + rng.integers(-128, 128, (len(up), 2)), -2**23, 2**23 - 1).astype(np.int32)
    raw = (x.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    return raw, x << 8  # the Q31 frames the reader hands out


def _f32_mono(tfp_lib, clip):
    x = (tfp_lib.resample_pcm(clip, 8000, 44100).astype(np.float64) / 32768.0 * 0.999).astype("<f4")
    return x.tobytes(), tfp_lib.q31_from_float(x).reshape(-1, 1)


def test_wide_files_are_enrolled_and_found(tfp_lib, tmp_path):
    from tiresias_amd import FpHandler
    from tiresias_amd.fp_handler import write_wav_mono16
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    d = tmp_path / "prompts"
    d.mkdir()
    # Two clips of resample_util.class_clip. The reference's search puts a box of the tolerance around the
    # integer part of each query frame's value, and a clip scores one per query frame that any of its rows meets.
    # On the CPU oracle, after these round trips, kind 0's inner frames lie at 18.17 to 18.21 and kind 1's at 17.38
    # to 17.42, so a query of kind 0 (box 17.55 to 18.45) meets no row of kind 1; but kind 0's first row, a partial
    # window, lies at 17.41, inside kind 1's box (16.55 to 17.45), so a query of kind 1 scores every frame on both
    # clips and the winner is decided by the random uuids. The second file is therefore searched for after the
    # first has been removed from the catalog.
    clips = [class_clip(k, 16000) for k in (0, 1)]
    raw24, q24 = _pcm24_stereo(tfp_lib, clips[0], 1)
    rawf, qf = _f32_mono(tfp_lib, clips[1])
    _write(d / "a_48k_stereo24.wav", 1, 24, 48000, 2, raw24)
    _write(d / "b_44k_float.wav", 3, 32, 44100, 1, rawf)
    host = {"a_48k_stereo24.wav": tfp_lib.resample_wide_pcm(q24, 2, 48000, 8000),
            "b_44k_float.wav": tfp_lib.resample_wide_pcm(qf, 1, 44100, 8000)}
    np.testing.assert_array_equal(tfp_lib.read_wav_interleaved_q31(str(d / "a_48k_stereo24.wav"))[0], q24)
    np.testing.assert_array_equal(tfp_lib.read_wav_interleaved_q31(str(d / "b_44k_float.wav"))[0], qf)

    h = FpHandler(0, index_rate=8000, mix_channels=True)  # without wide_samples: both refused, today's message
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        w0 = h.engine.resample_wide_stats()
        assert h.create_new_audio_info("ctx")
        assert h.fp_get_audio_lists_all() == [] and h.engine.resample_wide_stats() == w0
        assert "b_44k_float.wav" in h.last_error and "rate conversion takes 8/16-bit integer PCM and G.711 only" in h.last_error
        for name in host:
            h.last_error = ""
            assert h.fp_search_fingerprint_info("ctx", str(d / name), 1, 0.45, -1, -1) is None
            assert name in h.last_error and "rate conversion takes 8/16-bit integer PCM and G.711 only" in h.last_error
    finally:
        h.fp_term()

    h = FpHandler(0, index_rate=8000, wide_samples=True)  # several channels still need mix_channels
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        assert h.create_new_audio_info("ctx")
        assert [r["name"] for r in h.fp_get_audio_lists_all()] == ["b_44k_float.wav"]
        assert "a_48k_stereo24.wav" in h.last_error and "mix_channels" in h.last_error
    finally:
        h.fp_term()

    h = FpHandler(0, index_rate=8000, mix_channels=True, wide_samples=True)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        w0 = h.engine.resample_wide_stats()
        assert h.create_new_audio_info("ctx")
        w1 = h.engine.resample_wide_stats()
        # one launch per (channels, rate) group
        assert w1["launches"] - w0["launches"] == 2 and w1["frames_in"] - w0["frames_in"] == len(q24) + len(qf)
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert sorted(rows) == sorted(host)
        for name, pcm in host.items():
            m1, m2 = h.engine.index_rows(rows[name])
            ref = h.engine.fingerprint(pcm)  # the host route's rows
            assert np.array_equal(m1, ref["m1"]) and np.array_equal(m2, ref["m2"]), name
        for name, pcm in host.items():
            # found by the same audio at 8 kHz int16, as the host converter gives it
            q8 = tmp_path / ("q_" + name)
            write_wav_mono16(str(q8), pcm, 8000)
            got = h.fp_search_fingerprint_info("ctx", str(q8), 1, 0.45, -1, -1)
            assert got is not None and got["uuid"] == rows[name], name
            # and by the file itself: a file search converts on the host
            w2 = h.engine.resample_wide_stats()
            got = h.fp_search_fingerprint_info("ctx", str(d / name), 1, 0.45, -1, -1)
            assert got is not None and got["uuid"] == rows[name] and h.engine.resample_wide_stats() == w2
            assert got["frame_count"] == got["match_count"] == tfp_lib.frame_count(len(pcm))
            assert h.fp_delete_audio_list_info(rows[name])  # (see the note on the clips above)
        # a single file's enrolment converts on the host: the same rows
        d2 = tmp_path / "one"
        d2.mkdir()
        raw, q = _pcm24_stereo(tfp_lib, class_clip(2, 16000), 3)
        _write(d2 / "again.wav", 1, 24, 48000, 2, raw)
        w2 = h.engine.resample_wide_stats()
        assert h.fp_craete_audio_list_info("ctx", str(d2 / "again.wav"))
        assert h.engine.resample_wide_stats() == w2
        u = [r["uuid"] for r in h.fp_get_audio_lists_all() if r["name"] == "again.wav"][0]
        ref = h.engine.fingerprint(tfp_lib.resample_wide_pcm(q, 2, 48000, 8000))
        a, b = h.engine.index_rows(u)
        assert np.array_equal(a, ref["m1"]) and np.array_equal(b, ref["m2"])
    finally:
        h.fp_term()
