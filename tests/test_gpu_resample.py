"""Rate-normalised ingest on the GPU (tfp_fingerprint_rate_batch, tfp_search_rate_batch,
tfp_search_scoped_rate_batch): the frames of clips converted on the device equal, bit for bit, the int16
call over the host routine's output (tfp_resample_pcm) and the CPU oracle's fingerprint of it, at the
kernel's edges; the searches equal the pcm forms on the host-resampled queries."""
import ctypes as C

import numpy as np
import pytest

from fp_util import assert_frames_equal, launches_since
from resample_util import TILE, class_clip, bits_equal, edge_lengths, noise, ragged_order, rails

pytestmark = pytest.mark.gpu

# L = 1, M = 1, many phases, a table far larger than LDS; the last pair's span passes what a workgroup
# stages (a reduction by 64), so its tiles read their clip in global memory
PAIRS = [(16000, 8000), (48000, 8000), (8000, 16000), (44100, 8000), (11025, 8000), (8001, 8000), (64000, 1000)]
PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]
SEED_DB = 0x7153A1


@pytest.fixture(scope="module")
def eng(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    yield e
    e.close()


def _pack(clips):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    return (np.concatenate(clips) if clips else np.zeros(0, np.int16)).astype(np.int16), off


def _check_batch(eng, tfp_lib, oracle, clips, pair):
    """One batch through the rate form and through the int16 form over the host routine's output: equal
    frames, equal kernel choice, one conversion launch counted with its samples; -> the frames per clip."""
    rin, rout = pair
    pcm, off = _pack(clips)
    host = [tfp_lib.resample_pcm(c, rin, rout) for c in clips]
    hpcm, hoff = _pack(host)
    s0 = eng.fingerprint_stats()
    ref = eng.fingerprint_batch(hpcm, hoff, rout)
    d_ref = launches_since(eng, s0)
    r0, s1 = eng.resample_stats(), eng.fingerprint_stats()
    got = eng.fingerprint_rate_batch(pcm, off, rin, rout)
    d_got, r1 = launches_since(eng, s1), eng.resample_stats()
    assert d_got == d_ref, (d_got, d_ref)
    assert r1["launches"] - r0["launches"] == (1 if len(hpcm) else 0)
    assert r1["samples_in"] - r0["samples_in"] == (len(pcm) if len(hpcm) else 0)
    assert r1["samples_out"] - r0["samples_out"] == len(hpcm)
    bits_equal(got, ref)
    if len(hpcm):
        micro, db = oracle.fingerprint_batch(hpcm, hoff, rout, nthreads=8)
        assert_frames_equal(got, micro, db)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(h)) for h in host])])
    return [got[foff[i]:foff[i + 1]] for i in range(len(clips))]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_edges_single_and_ragged(eng, tfp_lib, oracle, pair):
    t = tfp_lib.resample_taps(*pair)
    lens = edge_lengths(t, TILE)
    single = {n: _check_batch(eng, tfp_lib, oracle, [noise(n, 7 + n)], pair)[0] for n in lens}
    order = ragged_order(lens)
    per_clip = _check_batch(eng, tfp_lib, oracle, [noise(n, 7 + n) for n in order], pair)
    for n, fr in zip(order, per_clip):  # a tile never reads its neighbour's samples
        bits_equal(fr, single[n])
    # the same batch further into the caller's buffer
    pcm, off = _pack([noise(n, 7 + n) for n in order])
    shifted = eng.fingerprint_rate_batch(np.concatenate([noise(333, 1), pcm]), off + 333, *pair)
    bits_equal(shifted, np.concatenate(per_clip))


@pytest.mark.parametrize("pair", PAIRS[:6], ids=lambda p: "%d-%d" % p)
def test_full_scale_clamp(eng, tfp_lib, oracle, pair):
    t = tfp_lib.resample_taps(*pair)
    run = max(t["M"], 8)  # at least four runs, so both rails are reached whatever M is
    x = rails(max(edge_lengths(t, TILE)[-1], 4 * run + 1), run)
    y = tfp_lib.resample_pcm(x, *pair)
    assert (y == 32767).any() and (y == -32768).any()
    _check_batch(eng, tfp_lib, oracle, [x], pair)


def test_large_batch_goes_through_device_memory(eng, tfp_lib, oracle):
    """Past the pinned staging's 8 MiB the samples are uploaded to a device buffer of their own."""
    clips = [noise(441000, 50 + i) for i in range(11)]  # 9.7 MB at 44.1 kHz
    _check_batch(eng, tfp_lib, oracle, clips, (44100, 8000))


def test_no_samples_no_launch(eng):
    r0 = eng.resample_stats()
    assert len(eng.fingerprint_rate_batch(np.zeros(0, np.int16), [0, 0, 0], 44100, 8000)) == 0
    assert len(eng.fingerprint_rate_batch(np.zeros(0, np.int16), [0], 44100, 8000)) == 0
    assert eng.resample_stats() == r0


def test_equal_rates_are_the_plain_form(eng):
    x = noise(5000, 2)
    r0 = eng.resample_stats()
    bits_equal(eng.fingerprint_rate_batch(x, [0, 1000, 5000], 8000, 8000), eng.fingerprint_batch(x, [0, 1000, 5000], 8000))
    assert eng.resample_stats() == r0


def _uuid(c):
    return "%08x-7a7e-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


@pytest.fixture(scope="module")
def db(tfp_lib, eng):
    """64 synthetic 8 kHz clips enrolled (scope c % 3), and 12 ragged excerpts of them."""
    nclips, n = 64, 8000 * 3
    e = tfp_lib.Engine(0)
    pcm = tfp_lib.synth_pcm(SEED_DB, range(nclips), n)
    fr = e.fingerprint_batch(pcm.reshape(-1), np.arange(nclips + 1, dtype=np.int64) * n)
    nf = tfp_lib.frame_count(n)
    uuids = [_uuid(c) for c in range(nclips)]
    for c in range(nclips):
        e.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    e.index_set_scope(uuids, [c % 3 for c in range(nclips)])
    rng = np.random.default_rng(11)
    cuts = [pcm[(5 * i) % nclips, 256 * (3 + i):256 * (3 + i) + 6000 + int(rng.integers(0, 4000))] for i in range(12)]
    yield e, pcm, uuids, cuts
    e.close()


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


@pytest.mark.parametrize("pair", [(16000, 8000), (44100, 8000)], ids=lambda p: "%d-%d" % p)
def test_searches_equal_the_pcm_forms(tfp_lib, db, pair):
    e, _, _, cuts = db
    rin, rout = pair
    qs = [tfp_lib.resample_pcm(c, rout, rin) for c in cuts] + [np.zeros(0, np.int16)]  # the excerpts at rate_in
    qpcm, qoff = _pack(qs)
    hpcm, hoff = _pack([tfp_lib.resample_pcm(q, rin, rout) for q in qs])
    scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
    found = 0
    for coefs, tol in PARAMS:
        p = tfp_lib.params(coefs, tol)
        r0 = e.resample_stats()
        res, fc = e.search_rate_batch(qpcm, qoff, rin, rout, p)
        assert e.resample_stats()["launches"] == r0["launches"] + 1
        ref, fc_ref = e.search_pcm_batch(hpcm, hoff, p, rout)
        assert [_key(r) for r in res] == [_key(r) for r in ref] and fc == fc_ref
        found += sum(r is not None for r in res)
        rows, rfc = e.search_scoped_rate_batch(qpcm, qoff, rin, rout, p, scopes, 3)
        assert rows == e.search_scoped_pcm_batch(hpcm, hoff, p, scopes, 3, rout)
        assert rfc == [tfp_lib.frame_count(int(hoff[i + 1] - hoff[i])) for i in range(len(qs))]
    assert found >= 1


def test_call_at_16k_against_an_8k_index(tfp_lib, oracle):
    """The purpose: excerpts of 8 enrolled 8 kHz clips heard at 16 kHz, searched with the rate form at
    (1, 0.45); the rows equal the CPU oracle's search of the host round trip."""
    nclips, n = 8, 8000 * 3
    e = tfp_lib.Engine(0)
    try:
        pcm = tfp_lib.synth_pcm(SEED_DB, range(nclips), n)
        off = np.arange(nclips + 1, dtype=np.int64) * n
        micro, _ = oracle.fingerprint_batch(pcm.reshape(-1), off, nthreads=8, want_db=False)
        nf = tfp_lib.frame_count(n)
        uuids = [_uuid(c) for c in range(nclips)]
        for c in range(nclips):
            e.index_add(uuids[c], micro[c * nf:(c + 1) * nf, 0], micro[c * nf:(c + 1) * nf, 1])
        clip = np.repeat(np.arange(nclips), nf)
        q16 = [tfp_lib.resample_pcm(pcm[i, 256 * (5 + i):256 * (5 + i) + 12000], 8000, 16000) for i in range(nclips)]
        qpcm, qoff = _pack(q16)
        res, _ = e.search_rate_batch(qpcm, qoff, 16000, 8000, tfp_lib.params(1, 0.45))
        found = 0
        for i in range(nclips):
            _, qdb, _ = oracle.fingerprint(tfp_lib.resample_pcm(q16[i], 16000, 8000))
            ok, w, mc, ofc = oracle.search(micro[:, 0], micro[:, 1], clip, uuids, qdb[:, 0], qdb[:, 1], 1, 0.45, -1, -1)
            assert _key(res[i]) == ((uuids[w], mc, ofc) if ok else None), i
            found += ok
        assert found >= 1
    finally:
        e.close()


@pytest.mark.parametrize("coefs", [1, 2])
def test_call_at_16k_names_the_right_clip(tfp_lib, oracle, coefs):
    """Identification, not only equality: excerpts heard at 16 kHz name their own 8 kHz clip at (coefs, 0.45).

    Three clips, not the issue's eight. The reference's search counts, per clip, the query frames whose box
    [k - tol, k + tol], k = (int)max1, holds one of the clip's rows, so a clip can win strictly only by rows
    in a box its rivals have none in. A CPU survey of 240 signals (tones of 100 .. 3000 Hz, alone and in
    noise of sigma 30 .. 4000) found frame values max1 of 16.5 .. 19.03 only, and three box classes that hold
    over a whole clip and survive the round trip: (18, 17), (17, 17) and (19, 16) (class_clip). The synthetic
    clips lie at max1 = 16.83 .. 16.88: k = 16, whose box [15.55, 16.45] misses their own rows, so an excerpt
    of one does not find it even without a conversion. With three classes at most three clips can each be
    named; every clip's zero-padded first frame also falls in box 17, so clip 1 and clip 0 count alike for
    clip 1's query and the reference's tie rule (the greater uuid) names clip 1."""
    nclips, n = 3, 8000 * 3
    e = tfp_lib.Engine(0)
    try:
        pcm = np.stack([class_clip(c, n) for c in range(nclips)])
        off = np.arange(nclips + 1, dtype=np.int64) * n
        micro, _ = oracle.fingerprint_batch(pcm.reshape(-1), off, nthreads=8, want_db=False)
        nf = tfp_lib.frame_count(n)
        uuids = [_uuid(c) for c in range(nclips)]
        for c in range(nclips):
            e.index_add(uuids[c], micro[c * nf:(c + 1) * nf, 0], micro[c * nf:(c + 1) * nf, 1])
        clip = np.repeat(np.arange(nclips), nf)
        q16 = [tfp_lib.resample_pcm(pcm[i, 256 * (5 + i):256 * (5 + i) + 12000], 8000, 16000) for i in range(nclips)]
        want = []
        for i in range(nclips):  # the condition first: the oracle's search of the host round trip names clip i
            _, qdb, _ = oracle.fingerprint(tfp_lib.resample_pcm(q16[i], 16000, 8000))
            ok, w, mc, ofc = oracle.search(micro[:, 0], micro[:, 1], clip, uuids, qdb[:, 0], qdb[:, 1], coefs, 0.45, -1, -1)
            assert ok and w == i and mc >= 40, (i, ok, w, mc)
            want.append((uuids[w], mc, ofc))
        qpcm, qoff = _pack(q16)
        res, _ = e.search_rate_batch(qpcm, qoff, 16000, 8000, tfp_lib.params(coefs, 0.45))
        assert [_key(r) for r in res] == want
    finally:
        e.close()


def test_equal_rate_searches_from_many_threads(tfp_lib, db):
    """Equal rates are the plain form, coalescer included: small searches through the rate form from many
    threads, beside plain pcm searches, all return (the rate form must not hold the engine's lock while it
    waits in the coalescer for a leader that needs it) and agree with the single-threaded answer."""
    import threading
    e, _, _, cuts = db
    p = tfp_lib.params(1, 0.45)
    want = [_key(e.search_pcm_batch(c, [0, len(c)], p)[0][0]) for c in cuts]
    got, errs = {}, []

    def work(t):
        try:
            for r in range(6):
                i = (t + r) % len(cuts)
                c = cuts[i]
                res = (e.search_rate_batch(c, [0, len(c)], 8000, 8000, p) if (t + r) % 2 == 0 else
                       e.search_pcm_batch(c, [0, len(c)], p))
                got[(t, r)] = (_key(res[0][0]), want[i])
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(60)
    assert not any(th.is_alive() for th in threads), "a search never returned"
    assert not errs, errs
    assert len(got) == 48 and all(a == b for a, b in got.values())


def test_error_paths_write_nothing(eng, tfp_lib):
    from tiresias_amd import _lib
    lib = tfp_lib.lib()
    x = noise(4000, 3)
    off = np.array([0, 4000], np.int64)
    p = tfp_lib.params(1, 0.45)
    scopes = np.array([-1], np.int32)
    r0 = eng.resample_stats()
    for rin, rout, msg in ((0, 8000, "bad sample rate"), (8000, -1, "bad sample rate"), (7999, 44100, "unsupported rate ratio")):
        frames = np.zeros(64, tfp_lib.FRAME_DTYPE)
        frames["m1"] = 77
        n = C.c_int64(-7)
        assert lib.tfp_fingerprint_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, rin, rout, frames.ctypes.data, 64,
                                              C.byref(n)) == -1
        assert msg in eng.last_error() and n.value == -7 and (frames["m1"] == 77).all()
        res = (_lib.Result * 1)()
        res[0].match_count = 77
        assert lib.tfp_search_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, rin, rout, C.byref(p), res) == -1
        assert msg in eng.last_error() and res[0].match_count == 77
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, rin, rout, C.byref(p),
                                                scopes.ctypes.data, 4, cand, cnt, fc) == -1
        assert msg in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    for k in (0, 1 << 20):
        cand, cnt, fc = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)
        assert lib.tfp_search_scoped_rate_batch(eng.handle, x.ctypes.data, off.ctypes.data, 1, 16000, 8000, C.byref(p),
                                                scopes.ctypes.data, k, cand, cnt, fc) == -1
        assert "k = " in eng.last_error() and cnt[0] == 7 and fc[0] == 7
    assert eng.resample_stats() == r0


# ---- the fp_handler mirror ---------------------------------------------------------------------

def test_mirror_normalises_to_its_index_rate(tfp_lib, tmp_path):
    """index_rate = 8000: a 16 kHz int16 WAV and a 16 kHz mu-law WAV are enrolled as their conversion (on the
    GPU), an 8 kHz WAV as it is, a 16 kHz stereo (fp32) WAV is refused with a message that says so; a file
    search of the 16 kHz file equals the search of its host conversion. index_rate = 0 behaves as before."""
    import wave
    from tiresias_amd import FpHandler
    from tiresias_amd.fp_handler import write_wav_mono16
    from g711_util import ULAW, encode, expand, g711_wav
    d = tmp_path / "prompts"
    d.mkdir()
    pcm = tfp_lib.synth_pcm(SEED_DB, range(4), 16000)
    wide = [tfp_lib.resample_pcm(pcm[i], 8000, 16000) for i in range(4)]
    write_wav_mono16(str(d / "a_8k.wav"), pcm[0])
    write_wav_mono16(str(d / "b_16k.wav"), wide[1], 16000)
    codes = encode(wide[2], ULAW)
    (d / "c_16k_ulaw.wav").write_bytes(g711_wav(codes, ULAW, 16000))
    with wave.open(str(d / "d_16k_stereo.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.stack([wide[3], wide[3] // 3], 1).astype("<i2").tobytes())
    h = FpHandler(0, index_rate=8000)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        r0 = h.engine.resample_stats()
        assert h.create_new_audio_info("ctx")
        r1 = h.engine.resample_stats()
        assert r1["launches"] - r0["launches"] == 1 and r1["samples_in"] - r0["samples_in"] == 2 * 32000
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert sorted(rows) == ["a_8k.wav", "b_16k.wav", "c_16k_ulaw.wav"]
        assert "d_16k_stereo.wav" in h.last_error and "fp32" in h.last_error and "16000" in h.last_error
        for name, src in (("a_8k.wav", pcm[0]), ("b_16k.wav", tfp_lib.resample_pcm(wide[1], 16000, 8000)),
                          ("c_16k_ulaw.wav", tfp_lib.resample_pcm(expand(codes, ULAW), 16000, 8000))):
            m1, m2 = h.engine.index_rows(rows[name])
            ref = h.engine.fingerprint(src)
            assert np.array_equal(m1, ref["m1"]) and np.array_equal(m2, ref["m2"]), name
        back = tfp_lib.resample_pcm(wide[1], 16000, 8000)
        want, _ = h.engine.search_pcm_batch(back, [0, len(back)], tfp_lib.params(1, 1.0))
        got = h.fp_search_fingerprint_info("ctx", str(d / "b_16k.wav"), 1, 1.0, -1, -1)
        assert got is not None and want[0] is not None
        assert (got["uuid"], got["match_count"], got["frame_count"]) == (want[0]["audio_uuid"], want[0]["match_count"],
                                                                        want[0]["frame_count"])
        h.last_error = ""
        assert h.fp_search_fingerprint_info("ctx", str(d / "d_16k_stereo.wav"), 1, 1.0, -1, -1) is None
        assert "fp32" in h.last_error
    finally:
        h.fp_term()
    h = FpHandler(0, index_rate=44100)  # 7999 -> 44100 has no table: the file is skipped, no row without frames
    assert h.fp_init()
    try:
        d2 = tmp_path / "odd"
        d2.mkdir()
        write_wav_mono16(str(d2 / "x_7999.wav"), pcm[0], 7999)
        assert h.fp_create_context_list_info("odd", str(d2), False) and h.create_new_audio_info("odd")
        assert h.fp_get_audio_lists_all() == [] and "unsupported rate ratio" in h.last_error
    finally:
        h.fp_term()
    h = FpHandler(0)  # native rates, as before: the 16 kHz file is enrolled at 16 kHz
    assert h.fp_init()
    try:
        assert h.index_rate == 0
        assert h.fp_create_context_list_info("ctx", str(d), False) and h.create_new_audio_info("ctx")
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert len(rows) == 4 and h.engine.resample_stats()["launches"] == 0
        m1, _ = h.engine.index_rows(rows["b_16k.wav"])
        assert np.array_equal(m1, h.engine.fingerprint(wide[1], 16000)["m1"])
    finally:
        h.fp_term()
