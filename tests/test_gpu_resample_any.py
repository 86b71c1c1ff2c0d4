"""Mixed batches on the GPU (tfp_fingerprint_any_batch, tfp_search_any_batch, tfp_search_scoped_any_batch): one call
whose clips each carry their own rate, channel count and sample kind gives, bit for bit, tfp_fingerprint_batch at
rate_out over each clip's tfp_resample_any_pcm, by ONE conversion launch whose tiles by form (staged, global, plain)
equal the counts the staging constants give, with the three single-class converters' and the G.711 counters
unmoved; it equals the per-class calls on the same clips; the searches equal the pcm forms on the host-mapped
queries; an argument error launches and writes nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_py
from resample_any_util import ALAW, Q31, S16, ULAW, class_map, form_of, key as _key, out_len, render, samples, tiles, uuid as _uuid
from resample_util import TILE, bits_equal, class_clip, in_len_for

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]


@pytest.fixture(scope="module")
def eng(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    yield e
    e.close()


def _older_stats(eng):
    return eng.resample_stats(), eng.resample_mix_stats(), eng.resample_wide_stats(), eng.g711_stats()


def _in_len(tfp_lib, n_out, rin, rout):
    if rin == rout:
        return n_out
    t = tfp_lib.resample_taps(rin, rout)
    return in_len_for(n_out, t["L"], t["M"]) if n_out else 0


def _edge_items(tfp_lib, classes, rout):
    """Every class at every output length, the classes interleaved so that consecutive tiles change class."""
    items = []
    for j, n_out in enumerate((0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE - 11)):
        for i, (kind, ch, rin) in enumerate(classes):
            x = samples(kind, _in_len(tfp_lib, n_out, rin, rout), ch, 100 * j + i)
            items.append((x, rin, kind))
    return items


def _check_call(eng, tfp_lib, items, rout, data=None, clips=None):
    """One mixed call against fingerprint_batch over every clip's host map: frames, the one launch, the tiles by
    form, the older counters; -> (frames, frame offsets per clip)."""
    if data is None:
        data, clips = tfp_lib.pack_audio_clips(items)
    host = [tfp_lib.resample_any_pcm(data, c, rout) for c in clips]
    for (x, rin, kind), h in zip(items, host):
        assert np.array_equal(h, class_map(tfp_lib, x, kind, rin, rout))
    hpcm = np.concatenate(host)
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int64)
    ref = eng.fingerprint_batch(hpcm, hoff, rout)
    want = dict(tiles_staged=0, tiles_global=0, tiles_plain=0)
    for (x, rin, kind), h in zip(items, host):
        assert len(h) == out_len(len(x), rin, rout)
        want["tiles_" + form_of(tfp_lib, kind, x.shape[1], rin, rout)] += tiles(len(h))
    a0, old0 = eng.resample_any_stats(), _older_stats(eng)
    got = eng.fingerprint_any_batch(data, clips, rout)
    a1 = eng.resample_any_stats()
    assert a1["launches"] - a0["launches"] == 1
    assert a1["clips"] - a0["clips"] == len(clips) and a1["samples_out"] - a0["samples_out"] == len(hpcm)
    assert a1["frames_in"] - a0["frames_in"] == sum(len(x) for x, _, _ in items)
    for k, v in want.items():
        assert a1[k] - a0[k] == v, (k, a1[k] - a0[k], v)
    assert _older_stats(eng) == old0
    bits_equal(got, ref)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(h)) for h in host])])
    return got, foff, host


EDGE_8K = [(S16, 1, 8000), (S16, 1, 16000), (S16, 2, 44100), (S16, 32, 16000), (Q31, 1, 48000), (Q31, 2, 44100),
           (Q31, 2, 96000), (Q31, 1, 192000), (ULAW, 1, 16000), (ALAW, 1, 8000)]


def test_edge_batch_at_8000(eng, tfp_lib):
    forms = [form_of(tfp_lib, k, ch, r, 8000) for k, ch, r in EDGE_8K]
    assert forms == ["plain", "staged", "staged", "staged", "staged", "staged", "global", "global", "staged", "plain"]
    items = _edge_items(tfp_lib, EDGE_8K, 8000)
    # an odd-length G.711 clip directly in front of a 4-byte aligned Q31 clip, and two descriptors naming the same bytes
    odd = samples(ULAW, 2 * TILE + 3, 1, 5)
    after = samples(Q31, 700, 2, 6)
    items += [(odd, 16000, ULAW), (after, 44100, Q31)]
    data, clips = tfp_lib.pack_audio_clips(items)
    assert int(clips["offset"][-1]) == int(clips["offset"][-2]) + len(odd) + 1 and int(clips["offset"][-1]) % 4 == 0
    twin = len(EDGE_8K) * 4 + 2  # the stereo 44100 clip of TILE + 1 outputs
    clips = np.concatenate([clips, clips[twin:twin + 1]])
    items.append(items[twin])
    got, foff, host = _check_call(eng, tfp_lib, items, 8000, data, clips)
    bits_equal(got[foff[-2]:foff[-1]], got[foff[twin]:foff[twin + 1]])
    # the CPU oracle on two of them: a staged Q31 stereo clip and a global Q31 mono clip of about three tiles
    for i in (len(EDGE_8K) * 5 + 5, len(EDGE_8K) * 5 + 7):
        micro, _ = oracle_py.fingerprint_batch(host[i], np.array([0, len(host[i])]), nthreads=2)
        mine = got[foff[i]:foff[i + 1]]
        assert len(mine) == len(micro) > 0
        assert np.array_equal(mine["m1"], micro[:, 0]) and np.array_equal(mine["m2"], micro[:, 1])


def test_second_call_at_16000(eng, tfp_lib):
    classes = [(ULAW, 1, 8000), (S16, 2, 44100), (S16, 1, 16000)]
    assert [form_of(tfp_lib, k, ch, r, 16000) for k, ch, r in classes] == ["staged", "staged", "plain"]
    _check_call(eng, tfp_lib, _edge_items(tfp_lib, classes, 16000), 16000)


def test_mixed_call_equals_the_per_class_calls(eng, tfp_lib):
    a, b = samples(S16, 5000, 1, 1), samples(S16, 3001, 1, 2)
    c, d = samples(S16, 9000, 2, 3), samples(S16, 77, 2, 4)
    w, v = samples(Q31, 12000, 3, 5), samples(Q31, 1, 3, 6)
    u = samples(ULAW, 4001, 1, 7)
    items = [(a, 16000, S16), (c, 44100, S16), (w, 48000, Q31), (u, 16000, ULAW), (b, 16000, S16), (d, 44100, S16),
             (v, 48000, Q31)]
    got, foff, _ = _check_call(eng, tfp_lib, items, 8000)
    part = lambda i: got[foff[i]:foff[i + 1]]  # noqa: E731
    bits_equal(np.concatenate([part(0), part(4)]),
               eng.fingerprint_rate_batch(np.concatenate([a, b]).reshape(-1), [0, len(a), len(a) + len(b)], 16000, 8000))
    bits_equal(np.concatenate([part(1), part(5)]),
               eng.fingerprint_mix_rate_batch(np.concatenate([c, d]), [0, len(c), len(c) + len(d)], 2, 44100, 8000))
    bits_equal(np.concatenate([part(2), part(6)]),
               eng.fingerprint_wide_rate_batch(np.concatenate([w, v]), [0, len(w), len(w) + len(v)], 3, 48000, 8000))
    bits_equal(part(3), eng.fingerprint_rate_batch(tfp_lib.decode_g711(u.reshape(-1), tfp_lib.ULAW), [0, len(u)], 16000, 8000))


def test_no_output_no_launch(eng, tfp_lib):
    a0 = eng.resample_any_stats()
    assert len(eng.fingerprint_any_batch(np.zeros(0, np.uint8), np.zeros(0, tfp_lib.CLIP_DTYPE), 8000)) == 0
    data, clips = tfp_lib.pack_audio_clips([(samples(S16, 0, 2, 1), 44100), (samples(ULAW, 0, 1, 1), 8000, ALAW)])
    assert len(eng.fingerprint_any_batch(data, clips, 8000)) == 0
    assert eng.resample_any_stats() == a0


@pytest.fixture(scope="module")
def db(tfp_lib, eng):
    """24 clips of 2 s at 8 kHz enrolled (scope c % 3): the three clips the reference's search tells apart
    (resample_util.class_clip) and synthetic ones; queries are excerpts of all of them."""
    n = 8000 * 2
    e = tfp_lib.Engine(0)
    clips = [class_clip(k, n) for k in (0, 1, 2)] + list(tfp_lib.synth_pcm(0x7153A1, range(21), n))
    uuids = [_uuid(c) for c in range(len(clips))]
    pcm = np.concatenate(clips)
    fr = e.fingerprint_batch(pcm, np.arange(len(clips) + 1) * n, 8000)
    nf = tfp_lib.frame_count(n)
    e.index_add_batch(uuids, np.arange(len(clips) + 1) * nf, fr["m1"], fr["m2"])
    e.index_set_scope(uuids, [c % 3 for c in range(len(clips))])
    cuts = [c[256 * (2 + i % 5):256 * (2 + i % 5) + 7000 + 300 * (i % 7)] for i, c in enumerate(clips)]
    yield e, cuts, uuids
    e.close()


def test_searches_equal_the_pcm_forms(tfp_lib, db):
    e, cuts, uuids = db
    items = [render(tfp_lib, c, i % 4, i) for i, c in enumerate(cuts)] + [(samples(Q31, 0, 2, 1), 48000, Q31)]
    data, clips = tfp_lib.pack_audio_clips(items)
    host = [tfp_lib.resample_any_pcm(data, c, 8000) for c in clips]
    hpcm = np.concatenate(host)
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int64)
    scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(items))]
    found = 0
    for coefs, tol in PARAMS:
        p = tfp_lib.params(coefs, tol)
        a0, old0 = e.resample_any_stats(), _older_stats(e)
        res, fc = e.search_any_batch(data, clips, 8000, p)
        a1 = e.resample_any_stats()
        assert a1["launches"] == a0["launches"] + 1 and _older_stats(e) == old0
        ref, fc_ref = e.search_pcm_batch(hpcm, hoff, p, 8000)
        assert [_key(r) for r in res] == [_key(r) for r in ref] and fc == fc_ref
        found += sum(r is not None and r["audio_uuid"] == uuids[i] for i, r in enumerate(res[:-1]))
        rows, rfc = e.search_scoped_any_batch(data, clips, 8000, p, scopes, 3)
        assert e.resample_any_stats()["launches"] == a1["launches"] + 1
        assert rows == e.search_scoped_pcm_batch(hpcm, hoff, p, scopes, 3, 8000)
        assert rfc == [tfp_lib.frame_count(len(h)) for h in host]
    assert found >= 1  # the searches are not vacuous: a class clip's excerpt names its clip


def test_argument_errors_launch_and_write_nothing(eng, tfp_lib):
    from tiresias_amd import _lib
    lib = tfp_lib.lib()
    good_items = [(samples(S16, 4000, 2, 3), 44100, S16), (samples(ULAW, 3000, 1, 4), 16000, ULAW)]
    data, good = tfp_lib.pack_audio_clips(good_items)
    p = tfp_lib.params(1, 0.45)
    scopes = np.array([-1] * 66, np.int32)

    def bad(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k][1] = v
        return c
    rates = np.zeros(65, tfp_lib.CLIP_DTYPE)
    rates["nframes"], rates["channels"], rates["rate_in"] = 8, 1, 8000 + 8 * np.arange(65)
    cases = [(bad(offset=int(good["offset"][1]) + 1, kind=S16), 8000, "clip 1: offset"), (bad(nframes=3001), 8000, "clip 1: reaches past"),
             (bad(offset=len(data) + 4, nframes=0), 8000, "clip 1: reaches past"), (rates, 8000, "clip 64: more than 64 distinct"),
             (bad(rate_in=7999), 44100, "clip 1: unsupported rate ratio 7999 -> 44100"), (bad(rate_in=0), 8000, "clip 1: bad sample rate"),
             (bad(channels=2), 8000, "clip 1: G.711 of 2 channels"), (bad(reserved=1), 8000, "clip 1: reserved")]
    a0, old0, f0 = eng.resample_any_stats(), _older_stats(eng), eng.fingerprint_stats()
    for clips, rout, msg in cases:
        n = len(clips)
        frames = np.zeros(64, tfp_lib.FRAME_DTYPE)
        frames["m1"] = 77
        got = C.c_int64(-7)
        assert lib.tfp_fingerprint_any_batch(eng.handle, data.ctypes.data, len(data), clips.ctypes.data, n, rout,
                                             frames.ctypes.data, 64, C.byref(got)) == -1
        assert msg in eng.last_error() and got.value == -7 and (frames["m1"] == 77).all(), eng.last_error()
        res = (_lib.Result * 66)()
        res[0].match_count = 77
        assert lib.tfp_search_any_batch(eng.handle, data.ctypes.data, len(data), clips.ctypes.data, n, rout, C.byref(p), res) == -1
        assert msg in eng.last_error() and res[0].match_count == 77
        cand, cnt, fc = (_lib.Candidate * 264)(), (C.c_int32 * 66)(7), (C.c_int32 * 66)(7)
        assert lib.tfp_search_scoped_any_batch(eng.handle, data.ctypes.data, len(data), clips.ctypes.data, n, rout, C.byref(p),
                                               scopes.ctypes.data, 4, cand, cnt, fc) == -1
        assert msg in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    # capacity: the need and nothing else; NULL data with frames to read
    frames = np.zeros(4, tfp_lib.FRAME_DTYPE)
    frames["m1"] = 77
    got = C.c_int64(-7)
    assert lib.tfp_fingerprint_any_batch(eng.handle, data.ctypes.data, len(data), good.ctypes.data, 2, 8000, frames.ctypes.data, 2,
                                         C.byref(got)) == -5
    need = sum(tfp_lib.frame_count(int(x)) for x in tfp_lib.audio_clips_check(good, len(data), 8000))
    assert got.value == need and (frames["m1"] == 77).all()
    assert lib.tfp_fingerprint_any_batch(eng.handle, None, len(data), good.ctypes.data, 2, 8000, frames.ctypes.data, 4,
                                         C.byref(got)) == -1 and "samples are NULL" in eng.last_error()
    assert eng.resample_any_stats() == a0 and _older_stats(eng) == old0 and eng.fingerprint_stats() == f0
    # a good call afterwards still succeeds
    _check_call(eng, tfp_lib, good_items, 8000)
