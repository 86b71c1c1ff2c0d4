"""Rate-normalised ingest of int32 Q31 frames on the GPU (tfp_fingerprint_wide_rate_batch,
tfp_search_wide_rate_batch, tfp_search_scoped_wide_rate_batch): the frames of interleaved Q31 clips converted on
the device equal, bit for bit, tfp_fingerprint_batch at rate_out over each clip's tfp_resample_wide_pcm, for every
form of the kernel (one channel staged as int32, several staged as int64 sums, the global-memory form past either
staging limit, the equal-rate form), with the form that ran read from tfp_resample_wide_stats; the searches equal
the pcm forms on the host-converted queries; an int16 batch widened by << 16 gives the mix form's frames."""
import ctypes as C

import numpy as np
import pytest

from fp_util import launches_since
from resample_util import TILE, bits_equal, class_clip, in_len_for, noise
from resample_wide_util import INT32_MAX, INT32_MIN, SPAN_MAX_MONO, SPAN_MAX_SUMS, pack, span_max, wide_noise

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]
SEED_DB = 0x7153A1


@pytest.fixture(scope="module")
def eng(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    yield e
    e.close()


def _expected_form(t, ch, pair):
    if pair[0] == pair[1]:
        return "downmix"
    return "staged" if span_max(t, TILE) <= (SPAN_MAX_MONO if ch == 1 else SPAN_MAX_SUMS) else "global"


def ragged_lengths(t, pair):
    """Frame counts of one ragged batch: none, one, shorter than the filter, exactly one tile of outputs, one
    output more, and a clip after one of odd length."""
    L, M = (1, 1) if pair[0] == pair[1] else (t["L"], t["M"])
    one_tile, more = in_len_for(TILE, L, M), in_len_for(TILE + 1, L, M)
    odd = 2 * t["ntaps"] + 1
    return [0, 1, t["ntaps"] - 1, one_tile, more, odd, 2 * t["ntaps"]]


def _check_batch(eng, tfp_lib, clips, ch, pair, form):
    """One batch through the wide form and through the int16 form over the host routine's output: equal frames,
    equal fingerprint kernel choice, one wide launch of the expected form counted with its frames, the other two
    converters' counters unmoved; -> the frames per clip."""
    rin, rout = pair
    q, off = pack(clips, ch)
    host = [tfp_lib.resample_wide_pcm(c, ch, rin, rout) for c in clips]
    hpcm = np.concatenate(host) if host else np.zeros(0, np.int16)
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int64)
    s0 = eng.fingerprint_stats()
    ref = eng.fingerprint_batch(hpcm, hoff, rout)
    d_ref = launches_since(eng, s0)
    w0, m0, r0, s1 = eng.resample_wide_stats(), eng.resample_mix_stats(), eng.resample_stats(), eng.fingerprint_stats()
    got = eng.fingerprint_wide_rate_batch(q, off, ch, rin, rout)
    d_got, w1 = launches_since(eng, s1), eng.resample_wide_stats()
    assert d_got == d_ref, (d_got, d_ref)
    ran = 1 if len(hpcm) else 0
    assert w1["launches"] - w0["launches"] == ran
    assert w1["staged_launches"] - w0["staged_launches"] == (ran if form in ("staged", "downmix") else 0), form
    assert w1["frames_in"] - w0["frames_in"] == (int(off[-1]) if ran else 0)
    assert w1["samples_out"] - w0["samples_out"] == len(hpcm)
    assert eng.resample_stats() == r0 and eng.resample_mix_stats() == m0
    bits_equal(got, ref)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(h)) for h in host])])
    return [got[foff[i]:foff[i + 1]] for i in range(len(clips))]


CASES = ([(1, p, "staged") for p in ((16000, 8000), (44100, 8000), (8000, 16000))] +
         [(ch, p, "staged") for ch in (2, 3, 5, 32) for p in ((48000, 8000), (44100, 8000))] +
         [(1, (96000, 8000), "staged"), (2, (96000, 8000), "global")] +
         [(1, (192000, 8000), "global"), (2, (192000, 8000), "global")] +
         [(1, (8000, 8000), "downmix"), (3, (8000, 8000), "downmix")])


@pytest.mark.parametrize("ch,pair,form", CASES, ids=lambda v: "%d-%d" % v if isinstance(v, tuple) else str(v))
def test_every_form_on_a_ragged_batch(eng, tfp_lib, ch, pair, form):
    t = tfp_lib.resample_taps(*pair)
    assert _expected_form(t, ch, pair) == form
    if pair == (96000, 8000):
        assert span_max(t, TILE) == 12854  # within the int32 limit, past the int64 one
    lens = ragged_lengths(t, pair)
    clips = [wide_noise(n, ch, 7 + n + ch) for n in lens]
    per_clip = _check_batch(eng, tfp_lib, clips, ch, pair, form)
    # a tile never reads its neighbour's frames: the two one-tile clips alone give the same frames
    for i in (3, 4):
        bits_equal(_check_batch(eng, tfp_lib, [clips[i]], ch, pair, form)[0], per_clip[i])
    # the same batch further into the caller's buffer
    q, off = pack(clips, ch)
    shifted = eng.fingerprint_wide_rate_batch(np.concatenate([wide_noise(333, ch, 1).reshape(-1), q]), off + 333, ch, *pair)
    bits_equal(shifted, np.concatenate(per_clip))


def test_full_scale_at_32_channels(eng, tfp_lib):
    for pair, form in (((44100, 8000), "staged"), ((8000, 8000), "downmix"), ((192000, 8000), "global")):
        t = tfp_lib.resample_taps(*pair)
        L, M = (1, 1) if pair[0] == pair[1] else (t["L"], t["M"])
        n = in_len_for(TILE + 37, L, M)
        lo, hi = np.full((n, 32), INT32_MIN, np.int32), np.full((n, 32), INT32_MAX, np.int32)
        alt = np.where(((np.arange(n) // max(20 * M // L, 8)) % 2 == 0)[:, None], hi, lo)  # runs of 20 outputs
        y = tfp_lib.resample_wide_pcm(alt, 32, *pair)
        assert (y == 32767).any() and (y == -32768).any()
        _check_batch(eng, tfp_lib, [lo, hi, alt], 32, pair, form)


def test_widened_int16_gives_the_mix_forms_frames(eng):
    for ch, pair in ((1, (44100, 8000)), (2, (44100, 8000)), (3, (8000, 16000)), (2, (8000, 8000)), (1, (8000, 8000))):
        x = noise(9000 * ch, 5 + ch)
        off = [0, 1001, 9000]
        wide = eng.fingerprint_wide_rate_batch(x.astype(np.int32) << 16, off, ch, *pair)
        bits_equal(wide, eng.fingerprint_mix_rate_batch(x, off, ch, *pair))


def test_no_frames_no_launch(eng):
    w0 = eng.resample_wide_stats()
    for pair in ((44100, 8000), (8000, 8000)):
        for ch in (1, 2):
            assert len(eng.fingerprint_wide_rate_batch(np.zeros(0, np.int32), [0, 0, 0], ch, *pair)) == 0
            assert len(eng.fingerprint_wide_rate_batch(np.zeros(0, np.int32), [0], ch, *pair)) == 0
    assert eng.resample_wide_stats() == w0


def test_error_paths_write_nothing(eng, tfp_lib):
    from tiresias_amd import _lib
    lib = tfp_lib.lib()
    x = wide_noise(4000, 2, 3)
    off = np.array([0, 4000], np.int64)
    p = tfp_lib.params(1, 0.45)
    scopes = np.array([-1], np.int32)
    w0, m0, r0 = eng.resample_wide_stats(), eng.resample_mix_stats(), eng.resample_stats()
    for ch, rin, rout, msg in ((0, 44100, 8000, "unsupported channel count"), (33, 44100, 8000, "unsupported channel count"),
                               (-2, 8000, 8000, "unsupported channel count"), (2, 0, 8000, "bad sample rate"),
                               (2, 8000, -1, "bad sample rate"), (2, 7999, 44100, "unsupported rate ratio")):
        frames = np.zeros(64, tfp_lib.FRAME_DTYPE)
        frames["m1"] = 77
        n = C.c_int64(-7)
        assert lib.tfp_fingerprint_wide_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout,
                                                   frames.ctypes.data, 64, C.byref(n)) == -1
        assert msg in eng.last_error() and n.value == -7 and (frames["m1"] == 77).all()
        res = (_lib.Result * 1)()
        res[0].match_count = 77
        assert lib.tfp_search_wide_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout, C.byref(p), res) == -1
        assert msg in eng.last_error() and res[0].match_count == 77
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_wide_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, ch, rin, rout, C.byref(p),
                                                     scopes.ctypes.data, 4, cand, cnt, fc) == -1
        assert msg in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    bad = np.array([0, 4000, 3000], np.int64)
    n = C.c_int64(-7)
    assert lib.tfp_fingerprint_wide_rate_batch(eng.handle, x.ctypes.data, bad.ctypes.data, 2, 2, 44100, 8000, None, 0,
                                               C.byref(n)) == -1
    assert "offsets not monotone" in eng.last_error() and n.value == -7
    for k in (0, 1 << 20):
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_wide_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, 2, 44100, 8000, C.byref(p),
                                                     scopes.ctypes.data, k, cand, cnt, fc) == -1
        assert "k = " in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    frames = np.zeros(4, tfp_lib.FRAME_DTYPE)
    frames["m1"] = 77
    n = C.c_int64(-7)
    assert lib.tfp_fingerprint_wide_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, 2, 44100, 8000, frames.ctypes.data,
                                               2, C.byref(n)) == -5  # TFP_E_CAPACITY: the need, nothing else
    assert n.value == tfp_lib.frame_count(tfp_lib.resample_count(4000, 44100, 8000)) and (frames["m1"] == 77).all()
    assert lib.tfp_fingerprint_wide_rate_batch(eng.handle, None, off.ctypes.data, 1, 2, 44100, 8000, frames.ctypes.data, 4,
                                               C.byref(n)) == -1
    assert eng.resample_wide_stats() == w0 and eng.resample_mix_stats() == m0 and eng.resample_stats() == r0


def _uuid(c):
    return "%08x-7a7e-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def _wide_stereo(tfp_lib, clip, rin, seed):
    """An 8 kHz int16 clip heard at rate_in on two Q31 channels: the clip plus and minus a difference signal, with
    the 16 bits below an int16 step filled, so the downmix is the clip to within the rounding."""
    up = tfp_lib.resample_pcm(clip, 8000, rin).astype(np.int64) << 16
    rng = np.random.default_rng(seed)
    side = rng.integers(-200 << 16, (200 << 16) + 1, len(up))
    fine = rng.integers(-2**15, 2**15, (len(up), 2))
    return np.clip(np.stack([up + side, up - side], 1) + fine, INT32_MIN, INT32_MAX).astype(np.int32)


@pytest.fixture(scope="module")
def db(tfp_lib, eng):
    """8 clips of 3 s at 8 kHz enrolled (scope c % 3): the three clips the reference's search tells apart
    (resample_util.class_clip) and five synthetic ones; queries are excerpts of all eight."""
    n = 8000 * 3
    e = tfp_lib.Engine(0)
    clips = [class_clip(k, n) for k in (0, 1, 2)] + list(tfp_lib.synth_pcm(SEED_DB, range(5), n))
    uuids = [_uuid(c) for c in range(len(clips))]
    for u, c in zip(uuids, clips):
        fr = e.fingerprint_batch(c, [0, n], 8000)
        e.index_add(u, fr["m1"], fr["m2"])
    e.index_set_scope(uuids, [c % 3 for c in range(len(clips))])
    cuts = [c[256 * (3 + i):256 * (3 + i) + 9000 + 700 * i] for i, c in enumerate(clips)]
    yield e, cuts, uuids
    e.close()


@pytest.mark.parametrize("pair", [(16000, 8000), (44100, 8000)], ids=lambda p: "%d-%d" % p)
def test_searches_equal_the_pcm_forms(tfp_lib, db, pair):
    e, cuts, uuids = db
    rin, rout = pair
    qs = [_wide_stereo(tfp_lib, c, rin, i) for i, c in enumerate(cuts)] + [np.zeros((0, 2), np.int32)]
    q, qoff = pack(qs, 2)
    host = [tfp_lib.resample_wide_pcm(x, 2, rin, rout) for x in qs]
    hpcm = np.concatenate(host)
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int64)
    scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
    found = 0
    for coefs, tol in PARAMS:
        p = tfp_lib.params(coefs, tol)
        w0 = e.resample_wide_stats()
        res, fc = e.search_wide_rate_batch(q, qoff, 2, rin, rout, p)
        w1 = e.resample_wide_stats()
        assert w1["launches"] == w0["launches"] + 1 and w1["staged_launches"] == w0["staged_launches"] + 1
        ref, fc_ref = e.search_pcm_batch(hpcm, hoff, p, rout)
        assert [_key(r) for r in res] == [_key(r) for r in ref] and fc == fc_ref
        found += sum(r is not None and r["audio_uuid"] == uuids[i] for i, r in enumerate(res))
        rows, rfc = e.search_scoped_wide_rate_batch(q, qoff, 2, rin, rout, p, scopes, 3)
        assert rows == e.search_scoped_pcm_batch(hpcm, hoff, p, scopes, 3, rout)
        assert rfc == [tfp_lib.frame_count(len(h)) for h in host]
    assert found >= 1  # the searches are not vacuous: a class clip's excerpt names its clip
