"""G.711 codes on the GPU: fingerprints, searches and stream ticks from mu-law / A-law codes.

The expansion is an exact integer map and the int16 kernels read its output unchanged, so nothing
here has a tolerance: every frame from codes is compared bit for bit (m1, m2, and q1 / q2 as bit
patterns) with fingerprint_batch of decode_g711(codes) and with the CPU oracle's fingerprint of the
same int16, and the path is asserted with the launch counters (Engine.fingerprint_stats must move
as it does for the int16 call; Engine.g711_stats counts the expansion where it is issued)."""
import numpy as np
import pytest

from fp_util import KERNELS, assert_frames_equal, assert_only_kernel, launches_since
from g711_util import ALAW, ULAW, encode, expand

pytestmark = pytest.mark.gpu

SEED_DB = 0x7153A1
LAWS = [pytest.param(ULAW, id="ulaw"), pytest.param(ALAW, id="alaw")]
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 513, 4001]
PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]


@pytest.fixture(scope="module")
def eng(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    yield e
    e.close()


def _bits_equal(a, b):
    """Frames from codes against frames from the expanded int16: every field, q as bit patterns."""
    assert len(a) == len(b)
    for k in ("frame_idx", "m1", "m2"):
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0][:10])
    for k in ("q1", "q2"):
        x, y = a[k].view(np.uint64), b[k].view(np.uint64)
        same = (x == y) | (np.isnan(a[k]) & np.isnan(b[k]))
        assert same.all(), (k, np.nonzero(~same)[0][:10])


def _check_batch(eng, oracle, codes, offsets, law, rate=8000):
    """One batch through the code form and the int16 form: equal frames, equal kernel choice, the
    expansion counted; -> the launches the int16 call made."""
    offsets = np.asarray(offsets, np.int64)
    pcm = expand(codes, law)
    total = int(offsets[-1] - offsets[0])
    s0 = eng.fingerprint_stats()
    ref = eng.fingerprint_batch(pcm, offsets, rate)
    d_ref = launches_since(eng, s0)
    g0, s1 = eng.g711_stats(), eng.fingerprint_stats()
    got = eng.fingerprint_g711_batch(codes, offsets, law, rate)
    d_got, g1 = launches_since(eng, s1), eng.g711_stats()
    assert d_got == d_ref, (d_got, d_ref)
    assert g1["codes"] - g0["codes"] == total
    assert g1["expand_launches"] - g0["expand_launches"] == (1 if total else 0)
    assert g1["stream_launches"] == g0["stream_launches"]
    _bits_equal(got, ref)
    micro, db = oracle.fingerprint_batch(pcm, offsets, rate, nthreads=8)
    assert_frames_equal(got, micro, db)
    return d_ref


def _ragged_lengths():
    """Three rounds of LENGTHS, the lengths that are 1 mod 16 first: the packed buffer's clip
    starts then run through every residue mod 16."""
    lens = LENGTHS * 3
    lens = [n for n in lens if n % 16 == 1] + [n for n in lens if n % 16 != 1]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert set(int(s) % 16 for s in starts) == set(range(16))
    return lens


@pytest.mark.parametrize("law", LAWS)
def test_every_code_bit_exact(eng, oracle, tfp_lib, law):
    rng = np.random.default_rng(7)
    codes = rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), 6))  # 1536 samples: 6 frames
    assert np.array_equal(tfp_lib.decode_g711(codes, law), expand(codes, law))
    d = _check_batch(eng, oracle, codes, [0, len(codes)], law)
    assert d["small8k"] == 1


@pytest.mark.parametrize("law", LAWS)
def test_ragged_small_batch(eng, oracle, law):
    lens = _ragged_lengths()
    codes = np.random.default_rng(11 + law).integers(0, 256, sum(lens)).astype(np.uint8)
    d = _check_batch(eng, oracle, codes, np.concatenate([[0], np.cumsum(lens)]), law)
    assert d["small8k"] == 1 and sum(d.values()) == 1


@pytest.mark.parametrize("law", LAWS)
def test_ragged_throughput_batch(eng, oracle, law):
    lens = (_ragged_lengths() * 10)[:300]
    codes = np.random.default_rng(13 + law).integers(0, 256, sum(lens)).astype(np.uint8)
    d = _check_batch(eng, oracle, codes, np.concatenate([[0], np.cumsum(lens)]), law)
    assert d["throughput8k"] >= 1 and d["small8k"] == 0 and d["generic_i16"] == 0


@pytest.mark.parametrize("law", LAWS)
def test_large_batch_goes_through_device_memory(eng, law):
    """More than 8 MiB of codes: they are uploaded to a device buffer of their own instead of the
    pinned staging. A smaller, different batch runs first, so frames left over in the engine's
    buffers cannot pass for this batch's."""
    n, nclips = 240000, 36  # 8.64 M codes
    base = np.random.default_rng(29 + law).integers(0, 256, n * 4).astype(np.uint8)
    codes = np.concatenate([np.roll(base, 977 * i)[:n] for i in range(nclips)])
    off = np.arange(nclips + 1, dtype=np.int64) * n
    assert len(codes) > (8 << 20)
    eng.fingerprint_g711_batch(codes[:n][::-1].copy(), [0, n], law)
    g0 = eng.g711_stats()
    got = eng.fingerprint_g711_batch(codes, off, law)
    g1 = eng.g711_stats()
    assert g1["expand_launches"] - g0["expand_launches"] == 1 and g1["codes"] - g0["codes"] == len(codes)
    eng.fingerprint_batch(expand(codes[:n][::-1].copy(), law), [0, n])
    _bits_equal(got, eng.fingerprint_batch(expand(codes, law), off))


@pytest.mark.parametrize("law", LAWS)
def test_offsets_need_not_start_at_zero(eng, oracle, law):
    codes = np.random.default_rng(17).integers(0, 256, 3000).astype(np.uint8)
    off = np.array([5, 5, 1030, 2999], np.int64)
    got = eng.fingerprint_g711_batch(codes, off, law)
    _bits_equal(got, eng.fingerprint_batch(expand(codes, law), off))


@pytest.mark.parametrize("law", LAWS)
def test_16k_takes_the_generic_kernel(eng, oracle, law):
    lens = _ragged_lengths()[:20]
    codes = np.random.default_rng(19 + law).integers(0, 256, sum(lens)).astype(np.uint8)
    s0 = eng.fingerprint_stats()
    _check_batch(eng, oracle, codes, np.concatenate([[0], np.cumsum(lens)]), law, rate=16000)
    assert_only_kernel(eng, s0, "generic_i16")


@pytest.mark.parametrize("law", LAWS)
def test_empty_batches(eng, law):
    g0, s0 = eng.g711_stats(), eng.fingerprint_stats()
    assert len(eng.fingerprint_g711_batch(np.zeros(0, np.uint8), [0, 0, 0], law)) == 0
    assert len(eng.fingerprint_g711_batch(np.zeros(0, np.uint8), [0], law)) == 0
    assert eng.g711_stats() == g0 and all(v == 0 for v in launches_since(eng, s0).values())


def test_bad_law_is_an_argument_error(eng, tfp_lib):
    codes = np.zeros(512, np.uint8)
    for call in (lambda: eng.fingerprint_g711_batch(codes, [0, 512], 2),
                 lambda: eng.search_g711_batch(codes, [0, 512], -1, tfp_lib.params(1, 0.45))):
        with pytest.raises(tfp_lib.TfpError) as e:
            call()
        assert e.value.code == -1 and "law" in str(e.value)


# ---- search ------------------------------------------------------------------------------------

class Db:
    pass


def _uuid(c):
    return "%08x-7110-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


@pytest.fixture(scope="module", params=LAWS)
def db(request, tfp_lib, oracle):
    """40 synthetic clips as codes of one law, their expansion and its oracle rows, and 16 queries
    cut from the expansion (on a hop boundary, so all but a cut's first frame are the clip's own) and
    re-encoded, packed so that every query but the first starts at an odd offset of the code buffer
    (host only; built once per law)."""
    law = request.param
    nclips, n = 40, 8000 * 3
    d = Db()
    d.law = law
    d.codes = encode(tfp_lib.synth_pcm(SEED_DB, range(nclips), n), law).reshape(nclips, n)
    d.pcm = expand(d.codes, law).reshape(nclips, n)
    d.off = np.arange(nclips + 1, dtype=np.int64) * n
    d.nf = (n + 255) // 256
    d.uuids = [_uuid(c) for c in range(nclips)]
    d.micro, _ = oracle.fingerprint_batch(d.pcm.reshape(-1), d.off, nthreads=8, want_db=False)
    d.clip = np.repeat(np.arange(nclips), d.nf)
    rng = np.random.default_rng(23)
    qs = []
    for i in range(16):
        a = 256 * int(rng.integers(0, (n - 9000) // 256))
        qs.append(encode(d.pcm[(i * 5) % nclips, a:a + (4097 if i == 0 else 4096) + 2 * int(rng.integers(0, 1500))], law))
    d.qcodes = np.concatenate(qs)
    d.qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
    assert all(int(o) % 2 == 1 for o in d.qoff[1:])
    d.qpcm = expand(d.qcodes, law)
    return d


def _enrol(e, d, frames):
    for c in range(len(d.uuids)):
        f = frames[c * d.nf:(c + 1) * d.nf]
        e.index_add(d.uuids[c], f["m1"], f["m2"])


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def test_search_from_codes(tfp_lib, oracle, db):
    a, b = tfp_lib.Engine(0), tfp_lib.Engine(0)
    try:
        fa = a.fingerprint_g711_batch(db.codes.reshape(-1), db.off, db.law)
        fb = b.fingerprint_batch(db.pcm.reshape(-1), db.off)
        _bits_equal(fa, fb)
        assert np.array_equal(fa["m1"], db.micro[:, 0]) and np.array_equal(fa["m2"], db.micro[:, 1])
        _enrol(a, db, fa)
        _enrol(b, db, fb)
        for u in db.uuids:  # enrolment from codes and from the expanded int16: identical rows
            ra, rb = a.index_rows(u), b.index_rows(u)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        found = 0
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            g0 = a.g711_stats()
            res, fc = a.search_g711_batch(db.qcodes, db.qoff, db.law, p)
            g1 = a.g711_stats()
            assert g1["expand_launches"] == g0["expand_launches"] + 1
            assert g1["codes"] - g0["codes"] == len(db.qcodes)
            ref, fc_ref = b.search_pcm_batch(db.qpcm, db.qoff, p)
            assert [_key(r) for r in res] == [_key(r) for r in ref] and fc == fc_ref
            for i in range(16):
                _, qdb, _ = oracle.fingerprint(db.qpcm[db.qoff[i]:db.qoff[i + 1]])
                ok, w, mc, ofc = oracle.search(db.micro[:, 0], db.micro[:, 1], db.clip, db.uuids, qdb[:, 0], qdb[:, 1],
                                               coefs, tol, -1, -1)
                assert _key(res[i]) == ((db.uuids[w], mc, ofc) if ok else None), (coefs, tol, i)
                found += ok
        assert found >= 1  # (not every comparison above was None against None)
    finally:
        a.close()
        b.close()


# ---- streams -----------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [255, 256, 4001])
def test_stream_mixed_ticks(tfp_lib, oracle, db, W):
    from tiresias_amd import Stream
    e = tfp_lib.Engine(0)
    try:
        _enrol(e, db, e.fingerprint_batch(db.pcm.reshape(-1), db.off))
        nch = 3
        st, twin = Stream(e, nch, W), Stream(e, nch, W)
        p = tfp_lib.params(1, 0.45)
        sizes = [1, 159, 160, 161, W]
        nticks = 15  # the 5 sizes x the 3 tick kinds; > 2 W samples: the ring wraps twice
        assert sum(sizes) * 3 > 2 * W + W
        # each channel plays an enrolled clip from an odd offset, as codes of both laws
        src = {law: encode(np.stack([db.pcm[7 * c + 1, 33 + c:33 + c + 16000] for c in range(nch)]), law)
               for law in (ULAW, ALAW)}
        hist = [np.zeros(0, np.int16) for _ in range(nch)]
        pos, code_ticks, full_checked = 0, 0, 0
        g0 = e.g711_stats()
        for t in range(nticks):
            T, kind = sizes[t % 5], t % 3  # int16 / mu-law / A-law
            law = ULAW if kind == 1 else ALAW
            codes = src[law][:, pos:pos + T]
            blk = expand(codes, law).reshape(nch, T)  # what the ring must hold for this tick
            pos += T
            if kind == 0:
                res = st.push(blk, p)
            else:
                res = st.push_g711(codes, law, p)
                code_ticks += 1
            ref = twin.push(blk, p)
            assert [_key(r) for r in res] == [_key(r) for r in ref], (t, T, kind)
            for c in range(nch):
                hist[c] = np.concatenate([hist[c], blk[c]])[-W:]
                fr = st.window_frames(c)
                if len(hist[c]) < W:
                    assert len(fr) == 0
                    continue
                _, qdb, micro = oracle.fingerprint(hist[c])
                assert_frames_equal(fr, micro, qdb)
                full_checked += 1
        g1 = e.g711_stats()
        assert g1["stream_launches"] - g0["stream_launches"] == code_ticks == 10
        assert g1["expand_launches"] == g0["expand_launches"]
        assert full_checked >= 3 * (nticks - 5)
        st.close()
        twin.close()
    finally:
        e.close()


# ---- device group ------------------------------------------------------------------------------

def test_group_equals_one_engine(tfp_lib, oracle, db):
    from tiresias_amd import Group, GroupStream, Stream
    g, e = Group([0, 0, 0]), tfp_lib.Engine(0)
    try:
        fe = e.fingerprint_g711_batch(db.codes.reshape(-1), db.off, db.law)
        fg = g.fingerprint_g711_batch(db.codes.reshape(-1), db.off, db.law)
        _bits_equal(fg, fe)
        _enrol(e, db, fe)
        for c in range(len(db.uuids)):
            f = fg[c * db.nf:(c + 1) * db.nf]
            g.index_add(db.uuids[c], f["m1"], f["m2"])
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            rg, fcg = g.search_g711_batch(db.qcodes, db.qoff, db.law, p)
            re_, fce = e.search_g711_batch(db.qcodes, db.qoff, db.law, p)
            assert [_key(r) for r in rg] == [_key(r) for r in re_] and fcg == fce
        # 192 equal-length queries: the group's query-sharded form (each shard expands its share)
        nq, qn = 192, 1024
        qc = np.ascontiguousarray(db.codes[:, 511:511 + qn * 5].reshape(-1)[:nq * qn])
        qo = np.arange(nq + 1, dtype=np.int64) * qn
        p = tfp_lib.params(1, 0.45)
        rg, _ = g.search_g711_batch(qc, qo, db.law, p)
        re_, _ = e.search_pcm_batch(expand(qc, db.law), qo, p)
        assert [_key(r) for r in rg] == [_key(r) for r in re_]
        # the same batch lying further into the caller's buffer (offsets[0] != 0), codes and int16:
        # the sharded form reads query i at offsets[i] of the buffer, as every other form does
        pad = 777
        qc2 = np.concatenate([np.full(pad, 0x55, np.uint8), qc])
        rg2, _ = g.search_g711_batch(qc2, qo + pad, db.law, p)
        assert [_key(r) for r in rg2] == [_key(r) for r in re_]
        rg3, _ = g.search_pcm_batch(expand(qc2, db.law), qo + pad, p)
        assert [_key(r) for r in rg3] == [_key(r) for r in re_]
        # stream ticks: codes and int16 mixed, the group against one engine
        nch, W = 3, 513
        gs, es = GroupStream(g, nch, W), Stream(e, nch, W)
        src = encode(np.stack([db.pcm[9 * c + 2, 101:101 + 4000] for c in range(nch)]), db.law)
        pos = 0
        for t, T in enumerate([161, 160, 159, 513, 1, 160, 161, 160]):
            codes = src[:, pos:pos + T]
            pos += T
            if t % 3 == 2:
                blk = expand(codes, db.law).reshape(nch, T)
                a, b = gs.push(blk, p), es.push(blk, p)
            else:
                a, b = gs.push_g711(codes, db.law, p), es.push_g711(codes, db.law, p)
            assert [_key(r) for r in a] == [_key(r) for r in b], t
        gs.close()
        es.close()
    finally:
        g.close()
        e.close()


def test_kernel_names_are_the_counters(eng):
    assert tuple(eng.fingerprint_stats()) == KERNELS
    assert tuple(eng.g711_stats()) == ("expand_launches", "stream_launches", "codes")


# ---- the fp_handler mirror ---------------------------------------------------------------------

def test_mirror_enrols_a_mixed_directory(tfp_lib, tmp_path):
    """One scan of a directory holding an int16 WAV, a mu-law WAV, headerless .ulaw and .alaw files
    and a stereo PCM WAV: the G.711 files go to the GPU as codes (one expansion per law), and each
    file is then found by a search of itself."""
    import wave
    from tiresias_amd import FpHandler
    from tiresias_amd.fp_handler import write_wav_mono16
    from g711_util import g711_wav
    d = tmp_path / "prompts"
    d.mkdir()
    pcm = tfp_lib.synth_pcm(SEED_DB, range(5), 16000)
    write_wav_mono16(str(d / "a_int16.wav"), pcm[0])
    (d / "b_tag7.wav").write_bytes(g711_wav(encode(pcm[1], ULAW), ULAW))
    (d / "c_raw.ulaw").write_bytes(encode(pcm[2], ULAW).tobytes())
    (d / "d_raw.alaw").write_bytes(encode(pcm[3], ALAW).tobytes())
    with wave.open(str(d / "e_stereo.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(np.stack([pcm[4], pcm[4] // 3], 1).astype("<i2").tobytes())
    h = FpHandler(0)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False)
        g0 = h.engine.g711_stats()
        assert h.create_new_audio_info("ctx")
        g1 = h.engine.g711_stats()
        assert g1["expand_launches"] - g0["expand_launches"] == 2  # one batch per law
        assert g1["codes"] - g0["codes"] == 3 * 16000
        rows = {r["name"]: r["uuid"] for r in h.fp_get_audio_lists_all()}
        assert sorted(rows) == ["a_int16.wav", "b_tag7.wav", "c_raw.ulaw", "d_raw.alaw", "e_stereo.wav"]
        # codes enrolled on the GPU leave the rows of their host expansion
        for name, law, clip in (("b_tag7.wav", ULAW, 1), ("c_raw.ulaw", ULAW, 2), ("d_raw.alaw", ALAW, 3)):
            m1, m2 = h.engine.index_rows(rows[name])
            ref = h.engine.fingerprint(expand(encode(pcm[clip], law), law))
            assert np.array_equal(m1, ref["m1"]) and np.array_equal(m2, ref["m2"]), name
        # Each file is found by a search of itself. A frame's box is [k - tol, k + tol] around k =
        # (int)max1 (fp_handler.c:287-351), and max1 lies in [k, k + 1) or (k - 1, k]: at tolerance 1
        # every frame with a max1 finds its own row, so the file itself has a match for each of them.
        # No clip can have more (a frame adds at most 1 to a clip), so the winner's count is that too.
        for name in rows:
            m1, _ = h.engine.index_rows(rows[name])
            own = int((m1 != tfp_lib.NULL_MICRO).sum())
            assert len(m1) == 63 and own > 0, name
            cands = h.fp_search_fingerprint_candidates("ctx", str(d / name), 1, 1.0, -1, -1, 5)
            mine = [c for c in cands if c["name"] == name]
            assert len(mine) == 1 and mine[0]["match_count"] == own and mine[0]["frame_count"] == 63, (name, own, cands)
            r = h.fp_search_fingerprint_info("ctx", str(d / name), 1, 1.0, -1, -1)
            assert r is not None and r["match_count"] == own and r["frame_count"] == 63, (name, r)
    finally:
        h.fp_term()
