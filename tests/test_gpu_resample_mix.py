"""Multichannel rate-normalised ingest on the GPU (tfp_fingerprint_mix_rate_batch, tfp_search_mix_rate_batch,
tfp_search_scoped_mix_rate_batch): the frames of interleaved clips downmixed and converted on the device
equal, bit for bit, the int16 call over the host routine's output (tfp_resample_mix_pcm) and the CPU
oracle's fingerprint of it, at the kernel's edges and on both sides of its staging budget; the searches
equal the pcm forms on the host-converted queries; the fp_handler mirror normalises multichannel files."""
import ctypes as C
import wave

import numpy as np
import pytest

from fp_util import assert_frames_equal, launches_since
from resample_mix_util import SPAN_MAX, mix_mean, mix_noise, pack, span_max
from resample_util import TILE, bits_equal, class_clip, edge_lengths, in_len_for, noise, ragged_order, rails

pytestmark = pytest.mark.gpu

PAIRS = [(16000, 8000), (44100, 8000), (8000, 16000)]
CHANNELS = [2, 3, 6]
PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]
SEED_DB = 0x7153A1


@pytest.fixture(scope="module")
def eng(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    yield e
    e.close()


def _check_batch(eng, tfp_lib, oracle, clips, ch, pair, staged=True):
    """One batch through the mix form and through the int16 form over the host routine's output: equal frames,
    equal fingerprint kernel choice, one mix launch of the expected form counted with its frames, the mono
    converter's counters unmoved; -> the frames per clip."""
    rin, rout = pair
    pcm, off = pack(clips, ch)
    host = [tfp_lib.resample_mix_pcm(c, ch, rin, rout) for c in clips]
    hpcm, hoff = pack(host, 1)
    s0 = eng.fingerprint_stats()
    ref = eng.fingerprint_batch(hpcm, hoff, rout)
    d_ref = launches_since(eng, s0)
    m0, r0, s1 = eng.resample_mix_stats(), eng.resample_stats(), eng.fingerprint_stats()
    got = eng.fingerprint_mix_rate_batch(pcm, off, ch, rin, rout)
    d_got, m1 = launches_since(eng, s1), eng.resample_mix_stats()
    assert d_got == d_ref, (d_got, d_ref)
    ran = 1 if len(hpcm) else 0
    assert m1["launches"] - m0["launches"] == ran
    assert m1["staged_launches"] - m0["staged_launches"] == (ran if staged else 0)
    assert m1["frames_in"] - m0["frames_in"] == (int(off[-1]) if ran else 0)
    assert m1["samples_out"] - m0["samples_out"] == len(hpcm)
    assert eng.resample_stats() == r0
    bits_equal(got, ref)
    if len(hpcm):
        micro, db = oracle.fingerprint_batch(hpcm, hoff, rout, nthreads=8)
        assert_frames_equal(got, micro, db)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(h)) for h in host])])
    return [got[foff[i]:foff[i + 1]] for i in range(len(clips))]


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_edges_single_and_ragged(eng, tfp_lib, oracle, pair, ch):
    t = tfp_lib.resample_taps(*pair)
    assert span_max(t, TILE) <= SPAN_MAX  # these pairs stage their channel sums
    lens = edge_lengths(t, TILE)
    single = {n: _check_batch(eng, tfp_lib, oracle, [mix_noise(n, ch, 7 + n)], ch, pair)[0] for n in lens}
    order = ragged_order(lens)
    clips = [mix_noise(n, ch, 7 + n) for n in order]
    starts = np.concatenate([[0], np.cumsum([len(c) * ch for c in clips])[:-1]])
    assert {int(s) % 2 for s in starts} == ({0, 1} if ch % 2 else {0})  # odd C: clip starts 2-byte aligned only
    per_clip = _check_batch(eng, tfp_lib, oracle, clips, ch, pair)
    for n, fr in zip(order, per_clip):  # a tile never reads its neighbour's frames
        bits_equal(fr, single[n])
    # the same batch further into the caller's buffer (an odd number of frames in: the other alignment)
    pcm, off = pack(clips, ch)
    shifted = eng.fingerprint_mix_rate_batch(np.concatenate([noise(333 * ch, 1), pcm]), off + 333, ch, *pair)
    bits_equal(shifted, np.concatenate(per_clip))


def _budget_pairs():
    """(rate_in, 8000) with the largest whole reduction whose tile span fits the staging budget, and the next."""
    def span(r):  # plan(8000 r, 8000): L = 1, M = r, ntaps = 48 r + 1
        return (TILE - 1) * r + 1 + 48 * r + 1
    r = max(r for r in range(2, 200) if span(r) <= SPAN_MAX)
    return (8000 * r, 8000), (8000 * (r + 1), 8000)


@pytest.mark.parametrize("side", ["within", "past"])
def test_both_sides_of_the_staging_budget(eng, tfp_lib, oracle, side):
    pair = _budget_pairs()[side == "past"]
    t = tfp_lib.resample_taps(*pair)
    staged = span_max(t, TILE) <= SPAN_MAX
    assert staged == (side == "within")
    n = in_len_for(TILE + 37, t["L"], t["M"])  # 2 tiles
    for ch in (2, 3):
        _check_batch(eng, tfp_lib, oracle, [mix_noise(n, ch, 5 + ch), mix_noise(3, ch, 1), mix_noise(n - 1, ch, 6 + ch)], ch,
                     pair, staged=staged)


@pytest.mark.parametrize("ch", [3, 32])
def test_full_scale_and_rails(eng, tfp_lib, oracle, ch):
    pair = (44100, 8000)
    t = tfp_lib.resample_taps(*pair)
    n = in_len_for(TILE + 37, t["L"], t["M"])
    r = np.repeat(rails(n, max(t["M"], 8))[:, None], ch, axis=1)
    y = tfp_lib.resample_mix_pcm(r, ch, *pair)
    assert (y == 32767).any() and (y == -32768).any()
    _check_batch(eng, tfp_lib, oracle, [np.full((n, ch), -32768, np.int16), np.full((n, ch), 32767, np.int16), r], ch, pair)
    _check_batch(eng, tfp_lib, oracle, [np.full((n, ch), -32768, np.int16)], ch, (8000, 16000))


@pytest.mark.parametrize("ch", [2, 3])
def test_a_neighbours_frames_never_leak(eng, ch):
    pair = (44100, 8000)
    n = 9001
    loud, quiet = np.full((n, ch), 32767, np.int16), np.zeros((n, ch), np.int16)
    alone = eng.fingerprint_mix_rate_batch(*pack([quiet], ch), ch, *pair)
    for clips, at in (([loud, quiet], 1), ([quiet, loud], 0), ([loud, quiet, loud], 1)):
        both = eng.fingerprint_mix_rate_batch(*pack(clips, ch), ch, *pair)
        k = len(both) // len(clips)
        bits_equal(both[at * k:(at + 1) * k], alone)


def test_one_channel_is_the_rate_form_and_equal_rates_downmix(eng, tfp_lib, oracle):
    x = noise(9000, 2)
    off = [0, 1000, 9000]
    m0, r0 = eng.resample_mix_stats(), eng.resample_stats()
    bits_equal(eng.fingerprint_mix_rate_batch(x, off, 1, 44100, 8000), eng.fingerprint_rate_batch(x, off, 44100, 8000))
    r1 = eng.resample_stats()
    assert r1["launches"] - r0["launches"] == 2 and eng.resample_mix_stats() == m0
    bits_equal(eng.fingerprint_mix_rate_batch(x, off, 1, 8000, 8000), eng.fingerprint_batch(x, off, 8000))
    assert eng.resample_stats() == r1 and eng.resample_mix_stats() == m0
    # equal rates, two channels: the downmix alone (no table, no filter), the integer mean
    for ch in (2, 3):
        clips = [mix_noise(n, ch, 40 + n) for n in (1, TILE - 1, TILE + 1, 2 * TILE + 1, 0, 300)]
        pcm, foff = pack(clips, ch)
        mean, moff = pack([mix_mean(c) for c in clips], 1)
        m0 = eng.resample_mix_stats()
        bits_equal(eng.fingerprint_mix_rate_batch(pcm, foff, ch, 8000, 8000), eng.fingerprint_batch(mean, moff, 8000))
        m1 = eng.resample_mix_stats()
        assert m1["launches"] - m0["launches"] == 1 and m1["staged_launches"] - m0["staged_launches"] == 1
        assert m1["frames_in"] - m0["frames_in"] == m1["samples_out"] - m0["samples_out"] == len(mean)
        assert eng.resample_stats() == r1


def test_no_frames_no_launch(eng):
    m0 = eng.resample_mix_stats()
    for pair in ((44100, 8000), (8000, 8000)):
        assert len(eng.fingerprint_mix_rate_batch(np.zeros(0, np.int16), [0, 0, 0], 2, *pair)) == 0
        assert len(eng.fingerprint_mix_rate_batch(np.zeros(0, np.int16), [0], 2, *pair)) == 0
    assert eng.resample_mix_stats() == m0


def test_error_paths_write_nothing(eng, tfp_lib):
    from tiresias_amd import _lib
    lib = tfp_lib.lib()
    x = mix_noise(4000, 2, 3)
    off = np.array([0, 4000], np.int64)
    p = tfp_lib.params(1, 0.45)
    scopes = np.array([-1], np.int32)
    m0, r0 = eng.resample_mix_stats(), eng.resample_stats()
    for ch, rin, rout, msg in ((0, 44100, 8000, "unsupported channel count"), (33, 44100, 8000, "unsupported channel count"),
                               (-2, 8000, 8000, "unsupported channel count"), (2, 0, 8000, "bad sample rate"),
                               (2, 8000, -1, "bad sample rate"), (2, 7999, 44100, "unsupported rate ratio")):
        frames = np.zeros(64, tfp_lib.FRAME_DTYPE)
        frames["m1"] = 77
        n = C.c_int64(-7)
        assert lib.tfp_fingerprint_mix_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout,
                                                  frames.ctypes.data, 64, C.byref(n)) == -1
        assert msg in eng.last_error() and n.value == -7 and (frames["m1"] == 77).all()
        res = (_lib.Result * 1)()
        res[0].match_count = 77
        assert lib.tfp_search_mix_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout, C.byref(p), res) == -1
        assert msg in eng.last_error() and res[0].match_count == 77
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_mix_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout, C.byref(p),
                                                    scopes.ctypes.data, 4, cand, cnt, fc) == -1
        assert msg in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    bad = np.array([0, 4000, 3000], np.int64)
    n = C.c_int64(-7)
    assert lib.tfp_fingerprint_mix_rate_batch(eng.handle, x.ctypes.data, bad.ctypes.data, 2, 2, 44100, 8000, None, 0,
                                              C.byref(n)) == -1
    assert "offsets not monotone" in eng.last_error() and n.value == -7
    for k in (0, 1 << 20):
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_mix_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, 2, 44100, 8000, C.byref(p),
                                                    scopes.ctypes.data, k, cand, cnt, fc) == -1
        assert "k = " in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    frames = np.zeros(4, tfp_lib.FRAME_DTYPE)
    frames["m1"] = 77
    n = C.c_int64(-7)
    assert lib.tfp_fingerprint_mix_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, 2, 44100, 8000, frames.ctypes.data,
                                              2, C.byref(n)) == -5  # TFP_E_CAPACITY: the need, nothing else
    assert n.value == tfp_lib.frame_count(tfp_lib.resample_count(4000, 44100, 8000)) and (frames["m1"] == 77).all()
    assert eng.resample_mix_stats() == m0 and eng.resample_stats() == r0


def _uuid(c):
    return "%08x-7a7e-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


@pytest.fixture(scope="module")
def db(tfp_lib, eng):
    """256 synthetic 8 kHz clips enrolled (scope c % 3), and 12 ragged excerpts of them."""
    nclips, n = 256, 8000 * 3
    e = tfp_lib.Engine(0)
    pcm = tfp_lib.synth_pcm(SEED_DB, range(nclips), n)
    fr = e.fingerprint_batch(pcm.reshape(-1), np.arange(nclips + 1, dtype=np.int64) * n)
    nf = tfp_lib.frame_count(n)
    uuids = [_uuid(c) for c in range(nclips)]
    foff = np.arange(nclips + 1, dtype=np.int64) * nf
    e.index_add_batch(uuids, foff, fr["m1"], fr["m2"])
    e.index_set_scope(uuids, [c % 3 for c in range(nclips)])
    rng = np.random.default_rng(11)
    cuts = [pcm[(5 * i) % nclips, 256 * (3 + i):256 * (3 + i) + 6000 + int(rng.integers(0, 4000))] for i in range(12)]
    yield e, cuts
    e.close()


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def _stereo(tfp_lib, cut, rin, seed):
    """An excerpt heard at rate_in on two channels: the clip itself plus and minus a small difference signal,
    so the downmix is the clip to within the rounding."""
    up = tfp_lib.resample_pcm(cut, 8000, rin).astype(np.int32)
    side = np.random.default_rng(seed).integers(-200, 201, len(up))
    return np.clip(np.stack([up + side, up - side], 1), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("pair", [(16000, 8000), (44100, 8000)], ids=lambda p: "%d-%d" % p)
def test_searches_equal_the_pcm_forms(tfp_lib, db, pair):
    e, cuts = db
    rin, rout = pair
    qs = [_stereo(tfp_lib, c, rin, i) for i, c in enumerate(cuts)] + [np.zeros((0, 2), np.int16)]
    qpcm, qoff = pack(qs, 2)
    hpcm, hoff = pack([tfp_lib.resample_mix_pcm(q, 2, rin, rout) for q in qs], 1)
    scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
    found = 0
    for coefs, tol in PARAMS:
        p = tfp_lib.params(coefs, tol)
        m0 = e.resample_mix_stats()
        res, fc = e.search_mix_rate_batch(qpcm, qoff, 2, rin, rout, p)
        assert e.resample_mix_stats()["launches"] == m0["launches"] + 1
        ref, fc_ref = e.search_pcm_batch(hpcm, hoff, p, rout)
        assert [_key(r) for r in res] == [_key(r) for r in ref] and fc == fc_ref
        found += sum(r is not None for r in res)
        rows, rfc = e.search_scoped_mix_rate_batch(qpcm, qoff, 2, rin, rout, p, scopes, 3)
        assert rows == e.search_scoped_pcm_batch(hpcm, hoff, p, scopes, 3, rout)
        assert rfc == [tfp_lib.frame_count(int(hoff[i + 1] - hoff[i])) for i in range(len(qs))]
    assert found >= 1


def _write_wav(path, x, rate, width=2):
    x = np.asarray(x)
    x = x.reshape(len(x), -1)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        if width == 2:
            w.writeframes(x.astype("<i2").tobytes())
        else:  # 24-bit: the int16 value in the upper two bytes
            w.writeframes((x.astype("<i4") << 8).view(np.uint8).reshape(-1, 4)[:, :3].tobytes())


def test_mirror_normalises_multichannel_files(tfp_lib, tmp_path):
    """index_rate = 8000 with mix_channels: a 44.1 kHz stereo 16-bit file and a 16 kHz mono file are enrolled as their conversion
    (one mix launch, one mono launch), a 44.1 kHz stereo 24-bit file is refused with the message that says what
    is taken; a search with the stereo file names it. Without mix_channels the stereo file is refused, as it
    was before the option. index_rate = 0: the stereo file goes through fp32."""
    from tiresias_amd import FpHandler
    from tiresias_amd.engine import read_wav_f32
    d = tmp_path / "prompts"
    d.mkdir()
    pcm = [class_clip(k, 16000) for k in (0, 2, 1)]  # clips the reference's search tells apart (resample_util)
    stereo = _stereo(tfp_lib, pcm[0], 44100, 1)
    mono16 = tfp_lib.resample_pcm(pcm[1], 8000, 16000)
    _write_wav(d / "a_44k_stereo.wav", stereo, 44100)
    _write_wav(d / "b_16k.wav", mono16, 16000)
    _write_wav(d / "c_44k_stereo24.wav", _stereo(tfp_lib, pcm[2], 44100, 2), 44100, width=3)
    h = FpHandler(0, index_rate=8000)  # the option is off by default: only the mono file is taken
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        m0 = h.engine.resample_mix_stats()
        assert h.create_new_audio_info("ctx")
        assert [r["name"] for r in h.fp_get_audio_lists_all()] == ["b_16k.wav"] and h.engine.resample_mix_stats() == m0
        assert "mix_channels" in h.last_error
        assert h.fp_search_fingerprint_info("ctx", str(d / "a_44k_stereo.wav"), 1, 0.45, -1, -1) is None
    finally:
        h.fp_term()
    h = FpHandler(0, index_rate=8000, mix_channels=True)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        m0, r0 = h.engine.resample_mix_stats(), h.engine.resample_stats()
        assert h.create_new_audio_info("ctx")
        m1, r1 = h.engine.resample_mix_stats(), h.engine.resample_stats()
        assert m1["launches"] - m0["launches"] == 1 and m1["frames_in"] - m0["frames_in"] == len(stereo)
        assert r1["launches"] - r0["launches"] == 1 and r1["samples_in"] - r0["samples_in"] == len(mono16)
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert sorted(rows) == ["a_44k_stereo.wav", "b_16k.wav"]
        assert "c_44k_stereo24.wav" in h.last_error and "44100" in h.last_error
        assert "rate conversion takes 8/16-bit integer PCM and G.711 only" in h.last_error
        for name, src in (("a_44k_stereo.wav", tfp_lib.resample_mix_pcm(stereo, 2, 44100, 8000)),
                          ("b_16k.wav", tfp_lib.resample_pcm(mono16, 16000, 8000))):
            m1_, m2_ = h.engine.index_rows(rows[name])
            ref = h.engine.fingerprint(src)  # the host route's rows
            assert np.array_equal(m1_, ref["m1"]) and np.array_equal(m2_, ref["m2"]), name
        got = h.fp_search_fingerprint_info("ctx", str(d / "a_44k_stereo.wav"), 1, 0.45, -1, -1)
        assert got is not None and got["uuid"] == rows["a_44k_stereo.wav"]
        assert got["frame_count"] == tfp_lib.frame_count(tfp_lib.resample_count(len(stereo), 44100, 8000))
        h.last_error = ""
        assert h.fp_search_fingerprint_info("ctx", str(d / "c_44k_stereo24.wav"), 1, 1.0, -1, -1) is None
        assert "8/16-bit integer PCM" in h.last_error
        # a single file's enrolment converts on the host: the same rows
        d2 = tmp_path / "one"
        d2.mkdir()
        _write_wav(d2 / "again.wav", _stereo(tfp_lib, pcm[2], 44100, 3), 44100)
        m2 = h.engine.resample_mix_stats()
        assert h.fp_craete_audio_list_info("ctx", str(d2 / "again.wav"))
        assert h.engine.resample_mix_stats() == m2
        u = [r["uuid"] for r in h.fp_get_audio_lists_all() if r["name"] == "again.wav"][0]
        ref = h.engine.fingerprint(tfp_lib.resample_mix_pcm(_stereo(tfp_lib, pcm[2], 44100, 3), 2, 44100, 8000))
        a, b = h.engine.index_rows(u)
        assert np.array_equal(a, ref["m1"]) and np.array_equal(b, ref["m2"])
    finally:
        h.fp_term()
    h = FpHandler(0, mix_channels=True)  # native rates, as before: the stereo file is enrolled at 44.1 kHz through the fp32 path
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        m0 = h.engine.resample_mix_stats()
        assert h.create_new_audio_info("ctx")
        assert h.engine.resample_mix_stats() == m0
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert sorted(rows) == ["a_44k_stereo.wav", "b_16k.wav", "c_44k_stereo24.wav"]
        x, sr = read_wav_f32(str(d / "a_44k_stereo.wav"))
        ref = h.engine.fingerprint_f32_batch(x, [0, len(x)], sr)
        a, b = h.engine.index_rows(rows["a_44k_stereo.wav"])
        assert sr == 44100 and np.array_equal(a, ref["m1"]) and np.array_equal(b, ref["m2"])
    finally:
        h.fp_term()
