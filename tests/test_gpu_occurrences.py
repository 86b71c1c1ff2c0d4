"""Diagonal trace and occurrence search (tfp_trace_batch, tfp_search_occurrences*, csrc/tfp_trace.hip,
csrc/tfp_occur.hpp): a clip laid on a recording at a start frame and verified along that one diagonal, and
the occurrences the rows of a sliding aligned search name, against the SQLite-derived fixture
tests/golden/occurrence_cases.json and occurrence_util's numpy reference over align_util.hit_matrix (the
oracle's frame boxes).

The kernel cuts a diagonal's frames into 64 contiguous chunks, one per lane, and joins the lanes' summaries
in lane order; the synthetic requests below take every start of every clip (1 to 300 rows) against a 700-frame
recording, so every overlap from 1 to 300 and every chunk length, clips that start before the recording and
run past its end, no overlap at all, and gaps of every length on the chunk borders."""
import ctypes as C

import numpy as np
import pytest

import align_util as A
import occurrence_util as O
import ranked_util as R
import scoped_util as S
import slide_align_util as SA

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_NOENT, TFP_E_CAPACITY = -1, -4, -5
ANY = -1
F_REC, OCC = 700, (123, 500)
SIZES = (1, 63, 64, 65, 128, 255, 256, 257, 120, 300)  # (the ninth: the all-equal clip)
EQUAL, LONG = 8, 9
GAPS = (0, 1, 3, 11, O.INT32_MAX)
# (coefs, tolerance, freq_ignore_low, freq_ignore_high): the last with keys 20, 21 below and 24, 25 above the thresholds
SETTINGS = ((1, 0.001, -1, -1), (2, 0.45, -1, -1), (2, 0.45, 150, 250))


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _uuid(c):
    return "00000000-0000-4000-8000-%012d" % c


def _six(t):
    return tuple(t[k] for k in O.TRACE_KEYS)


def _rows_of(wins_per_rec):
    """search_sliding_aligned_batch's result as occurrence_util's rows."""
    return [(r, row["audio_uuid"], w, row["offset"]) for r, wins in enumerate(wins_per_rec) for w, rows in enumerate(wins)
            for row in rows]


# ---- the goldens ------------------------------------------------------------------------------------------
def test_goldens_every_trace_and_list_engine_and_group(engine, tfp_lib):
    scen, _ = R.load_cases()
    g = tfp_lib.Group([0, 0])
    try:
        enrolled, traces, lists, found = None, 0, 0, 0
        for name, qi, window, hop, ctx, per in O.load_occurrences():
            s, q = scen[name], scen[name]["queries"][qi]
            col = {u: c for c, u in enumerate(s["uuids"])}
            if enrolled != name:
                S.enrol_scoped(engine, s)  # (after a clear the clip ids count from 0 in the scenario's order)
                S.enrol_scoped(g, s)
                enrolled = name
            fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
            for max_gap, min_hits, tr, occ in per:
                got = engine.trace_batch(fr, [0, len(fr)], p, [(0, col[u], st) for u, st, _n, _t in tr], max_gap)
                assert [_six(t) for t in got] == [t for _u, _st, _n, t in tr], (name, qi, window, hop, max_gap)
                traces += len(tr)
                for scopes in ([ctx], None) if ctx < 0 else ([ctx],):
                    one = engine.search_occurrences_batch(fr, [0, len(fr)], p, window, hop, SA.ROWS, max_gap, min_hits, scopes)
                    assert O.strip(one[0]) == occ, (name, qi, window, hop, ctx, max_gap, min_hits)
                    assert all(o["clip_id"] == col[o["audio_uuid"]] for o in one[0])
                    many = g.search_occurrences_batch(fr, [0, len(fr)], p, window, hop, SA.ROWS, max_gap, min_hits, scopes)
                    assert O.strip(many[0]) == occ, (name, qi, window, hop, ctx, max_gap, min_hits)
                    assert all(0 <= o["clip_id"] < 2 for o in many[0])  # clip_id is the shard
                    lists += 1
                    found += len(occ)
        assert traces > 1000 and lists >= 144 and found > 400
    finally:
        g.close()
        engine.index_clear()


# ---- the synthetic index ----------------------------------------------------------------------------------
def _synthetic():
    """(clips [(m1, m2)], q1, q2): clips of SIZES rows, max1 over 6 key values and max2 over 3, NULL rows in two of
    them, one all-equal clip, and clip-300 last (the greatest uuid); a 700-frame recording of the same values that
    holds clip-300 from frame 123 and again from frame 500 (its first 200 rows) with its rows 140-150 overwritten by
    a key no row has."""
    rng = np.random.default_rng(0x0CC5)
    clips = []
    for n in SIZES:
        m1 = rng.integers(20, 26, n).astype(np.int64) * 1_000_000 + 500
        m2 = rng.integers(5, 8, n).astype(np.int64) * 1_000_000
        clips.append((m1, m2))
    clips[EQUAL] = (np.full(120, 22_000_500, np.int64), np.full(120, 6_000_000, np.int64))
    clips[4][0][[0, 1, 57, 64, 127]] = R.NULL
    clips[4][1][[3, 57, 126]] = R.NULL
    clips[6][0][[63, 64, 128, 255]] = R.NULL
    k1, k2 = rng.integers(20, 26, F_REC), rng.integers(5, 8, F_REC)
    m1, m2 = clips[LONG]
    for at in OCC:
        n = min(300, F_REC - at)
        k1[at:at + n], k2[at:at + n] = m1[:n] // 1_000_000, m2[:n] // 1_000_000
    k1[OCC[1] + 140:OCC[1] + 151] = 30
    return clips, [float(v) + 0.2 for v in k1], [float(v) for v in k2]


@pytest.fixture(scope="module")
def synth(oracle):
    """The synthetic shapes' reference, computed once and left unchanged: per setting the hit matrix of the whole
    recording with every clip (align_util.hit_matrix), and per (setting, max_gap) the trace of every start of every
    clip (occurrence_util.trace_of_hits) with whether two segments tie for the best."""
    clips, q1, q2 = _synthetic()
    reqs = [(0, c, s) for c, (m1, _) in enumerate(clips) for s in range(-len(m1) - 10, F_REC + 11)]
    hits, ref = {}, {}
    for st in SETTINGS:
        hits[st] = [A.hit_matrix(oracle, m1, m2, q1, q2, *st) for m1, m2 in clips]
        for g in GAPS:
            ref[(st, g)] = [O.trace_of_hits(hits[st][c], s, g, more=True) for _, c, s in reqs]
    return clips, R.frames_from_q(q1, q2), reqs, hits, ref


def _enrol_synth(eng, clips):
    eng.index_clear()
    for c, (m1, m2) in enumerate(clips):  # (after a clear the clip ids count from 0 in this order)
        eng.index_add(_uuid(c), m1.astype(np.int32), m2.astype(np.int32))


def test_every_start_of_every_clip(engine, tfp_lib, synth):
    clips, rec, reqs, hits, ref = synth
    _enrol_synth(engine, clips)
    # what the requests cover, from the reference alone
    every = [t for st in SETTINGS for g in GAPS for t in ref[(st, g)]]
    assert sum(t[2] >= 2 for t, _ in every) >= 100                      # several segments
    assert sum(tie and t[2] >= 2 for t, tie in every) >= 10             # two segments tie for the best: the earlier is named
    assert any(t[0] == t[1] == 300 for t, _ in every)                   # an all-hit diagonal
    assert any(t[0] >= 20 and t[1] == 0 for t, _ in every)              # a no-hit diagonal
    assert {t[0] for t, _ in ref[(SETTINGS[0], 0)]} == set(range(301))  # every overlap, none included
    # gaps of exactly max_gap and max_gap + 1 between two hits (one segment, two segments), at every place of a chunk
    h, gaps = hits[SETTINGS[0]][LONG], set()
    for s in range(-200, F_REC, 7):
        xs = np.arange(max(0, s), min(F_REC, s + 300))
        gaps |= set((np.diff(xs[h[xs, xs - s]]) - 1).tolist())
    assert {g + d for g in GAPS[:4] for d in (0, 1)} <= gaps
    for st in SETTINGS:
        p = tfp_lib.params(*st)
        for g in GAPS:
            before = engine.trace_stats()
            got = engine.trace_batch(rec, [0, F_REC], p, reqs, g)
            after = engine.trace_stats()
            exp = [t for t, _ in ref[(st, g)]]
            bad = [(reqs[i], _six(got[i]), exp[i]) for i in range(len(reqs)) if _six(got[i]) != exp[i]]
            assert not bad, (st, g, len(bad), bad[:5])
            # one launch, the requests with an overlap computed there and the rest answered on the host
            assert (after["batches"] - before["batches"], after["traces"] - before["traces"]) == (1, sum(t[0] > 0 for t in exp))
    engine.index_clear()


def test_occurrences_of_the_two_playings(engine, tfp_lib, synth):
    clips, rec, _reqs, hits, _ref = synth
    _enrol_synth(engine, clips)
    col = {_uuid(c): c for c in range(len(clips))}
    collapsed, k = 0, len(clips)  # (every clip with a hit is a row: the all-equal clip's count is low)
    for st in SETTINGS[:2]:
        p = tfp_lib.params(*st)
        for window in (48, 24):
            rows = _rows_of(engine.search_sliding_aligned_batch(rec, [0, F_REC], p, window, 6, k))
            named = O.candidates_of_rows(rows, 6)
            for max_gap in (0, 3, 11, 40, O.INT32_MAX):
                for min_hits in (1, 20):
                    exp = O.occurrences_of_rows(rows, 6, lambda _r, u, s: O.trace_of_hits(hits[st][col[u]], s, max_gap), min_hits)
                    sa, tr = engine.slide_align_stats(), engine.trace_stats()
                    got = engine.search_occurrences_batch(rec, [0, F_REC], p, window, 6, k, max_gap, min_hits)[0]
                    sa2, tr2 = engine.slide_align_stats(), engine.trace_stats()
                    assert O.strip(got) == exp, (st, window, max_gap, min_hits)
                    # the trace kernel computed the distinct candidates, once each
                    assert (tr2["batches"] - tr["batches"], tr2["traces"] - tr["traces"]) == (1, len(named))
                    # and the sliding alignment moved as the sliding aligned call alone moves it
                    engine.search_sliding_aligned_batch(rec, [0, F_REC], p, window, 6, k)
                    sa3 = engine.slide_align_stats()
                    assert {k: sa2[k] - sa[k] for k in sa} == {k: sa3[k] - sa2[k] for k in sa}
                    long = [o for o in got if o["audio_uuid"] == _uuid(LONG)]
                    first = next(o for o in long if o["clip_start_frame"] == 123)
                    assert (first["first_frame"], first["last_frame"], first["hits"], first["overlap"]) == (123, 422, 300, 300)
                    assert first["diagonal_hits"] == 300 and first["windows"] >= 2
                    second = next(o for o in long if o["clip_start_frame"] == 500)
                    assert (second["overlap"], second["diagonal_hits"]) == (200, 189)
                    if max_gap >= 11:  # rows 140-150 are a gap of 11 frames: one segment
                        assert (second["first_frame"], second["last_frame"], second["hits"]) == (500, 699, 189)
                    else:              # two segments, the first the best
                        assert (second["first_frame"], second["last_frame"], second["hits"]) == (500, 639, 140)
                    # the all-equal clip: its tied starts collapse to disjoint intervals
                    eq = [o for o in got if o["audio_uuid"] == _uuid(EQUAL)]
                    n_eq = sum(u == _uuid(EQUAL) for _r, u, _s in named)
                    collapsed += n_eq - len(eq)
                    assert all(a["last_frame"] < b["first_frame"] for a, b in zip(eq, eq[1:]))
    assert collapsed > 50
    engine.index_clear()


def test_group_equals_one_engine_over_several_recordings(engine, tfp_lib, synth):
    clips, rec, _reqs, _hits, _ref = synth
    g = tfp_lib.Group([0, 0])
    try:
        _enrol_synth(engine, clips)
        _enrol_synth(g, clips)
        recs = np.concatenate([rec[100:460], rec[:30], rec[480:]])
        qoff = [0, 360, 390, 390 + 220]
        p = tfp_lib.params(1, 0.001)
        want = engine.search_occurrences_batch(recs, qoff, p, 48, 6, 4, 11, 5)
        got = g.search_occurrences_batch(recs, qoff, p, 48, 6, 4, 11, 5)
        assert [O.strip(r) for r in got] == [O.strip(r) for r in want]
        assert want[1] == [] and len(want[0]) >= 1 and len(want[2]) >= 1  # (the second recording is shorter than the window)
        assert {o["clip_start_frame"] for o in want[0] if o["audio_uuid"] == _uuid(LONG)} >= {23}
        assert {o["clip_id"] for r in got for o in r} == {0, 1}  # both shards hold an occurrence's clip
    finally:
        g.close()
        engine.index_clear()


def test_pcm_form_equals_the_frames_form(engine, tfp_lib):
    n = 8000 * 4
    pcm = tfp_lib.synth_pcm(0x7153A1, range(3), n)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(4) * n)
    nf = len(fr) // 3
    uuids = [_uuid(i) for i in range(3)]
    engine.index_clear()
    for c in range(3):
        engine.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    engine.index_set_scope(uuids, [3, 4, 3])
    noise = tfp_lib.synth_pcm(0xBEEF, range(3), 6000)
    recs = [np.concatenate([noise[i][:256 * (3 + i)], pcm[i][256 * 20:256 * 20 + ln], noise[i][:1000 + 300 * i]])
            for i, ln in enumerate((12000, 7000 + 77, 3000))]
    flat = np.concatenate(recs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    rfr = engine.fingerprint_batch(flat, off)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(r)) for r in recs])])
    seen = 0
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        for window, hop in ((12, 5), (12, 7)):
            for scopes in (None, [3, 4, ANY]):
                for max_gap, min_hits in ((8, 1), (2, 2)):
                    got = engine.search_occurrences_pcm_batch(flat, off, p, window, hop, 3, max_gap, min_hits, scopes)
                    assert got == engine.search_occurrences_batch(rfr, foff, p, window, hop, 3, max_gap, min_hits, scopes), \
                        (p.coefs, window, hop, max_gap)
                    seen += sum(len(r) for r in got)
    assert seen > 4
    engine.index_clear()


def test_a_clip_of_the_index_delta_is_traced(tfp_lib, monkeypatch, synth):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    clips, rec, reqs, _hits, ref = synth
    st, p = SETTINGS[0], tfp_lib.params(*SETTINGS[0])
    with tfp_lib.Engine(0) as eng:
        for c in range(LONG):
            eng.index_add(_uuid(c), clips[c][0].astype(np.int32), clips[c][1].astype(np.int32))
        eng.index_commit()
        eng.search_ranked_batch(R.frames_from_q([24.3], [1.0]), [0, 1], p, 1)
        eng.index_add(_uuid(LONG), clips[LONG][0].astype(np.int32), clips[LONG][1].astype(np.int32))  # after the build
        mine = [i for i, r in enumerate(reqs) if r[1] == LONG]
        got = eng.trace_batch(rec, [0, F_REC], p, [reqs[i] for i in mine], 3)
        assert [_six(t) for t in got] == [ref[(st, 3)][i][0] for i in mine]
        occ = eng.search_occurrences_batch(rec, [0, F_REC], p, 48, 6, 4, 11, 20)[0]
        assert eng.index_delta_stats()[1] == 1  # served beside the index, no merge
        assert {123, 500} <= {o["clip_start_frame"] for o in occ if o["audio_uuid"] == _uuid(LONG)}


def test_contract(engine, tfp_lib, synth):
    from tiresias_amd._lib import Occurrence, Trace, TraceReq
    clips, rec, _reqs, _hits, _ref = synth
    _enrol_synth(engine, clips)
    L = tfp_lib.lib()
    p = tfp_lib.params(1, 0.001)
    fr = rec[100:300]

    def raw_occ(window=48, hop=6, k=4, scope=ANY, cap=64, qoff=(0, 200), pp=p, max_gap=3, min_hits=2):
        out, n = (Occurrence * max(cap, 1))(), C.c_int64(-7)
        C.memset(out, 0xFF, C.sizeof(out))
        qo, sc = (C.c_int64 * len(qoff))(*qoff), (C.c_int32 * len(qoff))(*[scope] * len(qoff))
        rc = L.tfp_search_occurrences_batch(engine.handle, fr.ctypes.data, qo, len(qoff) - 1, C.byref(pp), window, hop, sc, k,
                                            max_gap, min_hits, out, cap, C.byref(n))
        return rc, n.value, bytes(out) == b"\xff" * C.sizeof(out), out

    def raw_trace(reqs=((0, LONG, 23),), qoff=(0, 200), pp=p, max_gap=3):
        rq, out = (TraceReq * max(len(reqs), 1))(), (Trace * max(len(reqs), 1))()
        for i, (r, c, s) in enumerate(reqs):
            rq[i] = TraceReq(r, c, s, 0)
        C.memset(out, 0xFF, C.sizeof(out))
        qo = (C.c_int64 * len(qoff))(*qoff)
        rc = L.tfp_trace_batch(engine.handle, fr.ctypes.data, qo, len(qoff) - 1, C.byref(pp), rq, len(reqs), max_gap, out)
        return rc, bytes(out) == b"\xff" * C.sizeof(out), out

    rc, n, untouched, out = raw_occ()
    assert rc == 0 and 1 <= n <= 64 and not untouched
    assert any(out[i].uuid.decode() == _uuid(LONG) and out[i].clip_start_frame == 23 for i in range(n))
    # too little room: *noccurrences is set and nothing else written
    for cap in (n - 1, 0):
        assert raw_occ(cap=cap)[:3] == (TFP_E_CAPACITY, n, True)
    assert raw_occ(cap=n)[:2] == (0, n)
    # each argument case: the sliding call's, and max_gap and min_hits
    for kw in (dict(window=0), dict(window=-3), dict(hop=0), dict(hop=-1), dict(k=0), dict(k=33),
               dict(pp=tfp_lib.params(3, 0.001)), dict(pp=tfp_lib.params(0, 0.001)), dict(qoff=(0, 120, 80)), dict(scope=-2),
               dict(max_gap=-1), dict(min_hits=0), dict(min_hits=-5)):
        rc, _n, untouched, _ = raw_occ(**kw)
        assert rc == TFP_E_ARG and untouched, kw
    rc, untouched, out = raw_trace(reqs=((0, LONG, 23), (0, -1, 0), (0, 0, 500), (0, LONG, -2 ** 31), (0, LONG, 2 ** 31 - 1)))
    assert rc == 0 and _six_raw(out[0])[:2] == (177, 177)
    assert [_six_raw(out[i]) for i in range(1, 5)] == [(0,) * 6] * 4  # no clip, and no overlap at any int32 start
    for kw in (dict(max_gap=-1), dict(pp=tfp_lib.params(3, 0.001)), dict(qoff=(0, 120, 80)), dict(reqs=((1, LONG, 0),)),
               dict(reqs=((0, LONG, 0), (-1, LONG, 0)))):
        rc, untouched, _ = raw_trace(**kw)
        assert rc == TFP_E_ARG and untouched, kw
    for bad in (len(clips), -2, 1 << 30):
        rc, untouched, _ = raw_trace(reqs=((0, LONG, 23), (0, bad, 0)))
        assert rc == TFP_E_NOENT and untouched, bad
    engine.index_remove(_uuid(2))
    rc, untouched, _ = raw_trace(reqs=((0, 2, 0),))
    assert rc == TFP_E_NOENT and untouched
    # nothing to trace, a recording shorter than the window, no recording: nothing is launched
    before = (engine.trace_stats(), engine.slide_align_stats())
    assert raw_trace(reqs=())[0] == 0
    assert raw_trace(reqs=((0, -1, 5), (0, LONG, 200), (0, LONG, -300)))[0] == 0
    assert raw_occ(window=201)[:3] == (0, 0, True)
    assert engine.search_occurrences_batch(fr, [0, 5, 5, 40], p, 48, 6, 2, 3, 1) == [[], [], []]
    assert engine.search_occurrences_batch(np.zeros(0, R.FRAME_DTYPE), [0], p, 48, 6, 2, 3, 1) == []
    # an empty index: the windows are there, no row, nothing launched
    engine.index_clear()
    assert raw_occ()[:3] == (0, 0, True)
    assert (engine.trace_stats(), engine.slide_align_stats()) == before
    b, t = C.c_int64(-1), C.c_int64(-1)
    assert L.tfp_trace_stats(engine.handle, None, None) == 0
    assert L.tfp_trace_stats(engine.handle, C.byref(b), C.byref(t)) == 0 and min(b.value, t.value) >= 0


def _six_raw(t):
    return (t.overlap, t.hits, t.segments, t.seg_hits, t.seg_first, t.seg_last)
