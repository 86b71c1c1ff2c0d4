"""Sliding search (tfp_search_sliding*, csrc/tfp_slide.hip): for every window of a recording the first k
rows of the reference's result query (fp_handler.c:367-374) over that window's frames, against the
SQLite-peeled per-window fixture tests/golden/sliding_cases.json, the oracle's brute-force count, and
search_scoped_batch / search_ranked_batch (unchanged code) called on the explicit windows."""
import ctypes as C
import math

import numpy as np
import pytest

import ranked_util as R
import scoped_util as S
import sliding_util as W

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
ANY = -1
RUN = 32  # TFP_SLIDE_RUN, asserted against the binding below


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _batch(frames):
    return (np.concatenate(frames) if frames else np.zeros(0, R.FRAME_DTYPE),
            np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64))


def _explicit(eng, recs, p, window, hop, scopes, k):
    """The definition: every window cut out and searched as a query of its own, by the scoped batch
    (the ranked batch without scopes). Per recording a list of per-window row lists."""
    cuts, cs, per = [], [], []
    for r, fr in enumerate(recs):
        n = W.nwin(len(fr), window, hop)
        per.append(n)
        for w in range(n):
            cuts.append(fr[w * hop:w * hop + window])
            cs.append(ANY if scopes is None else scopes[r])
    if not cuts:
        return [[] for _ in recs]
    fr, qoff = _batch(cuts)
    rows = eng.search_ranked_batch(fr, qoff, p, k) if scopes is None else eng.search_scoped_batch(fr, qoff, p, cs, k)
    off = np.concatenate([[0], np.cumsum(per)])
    return [rows[off[r]:off[r + 1]] for r in range(len(recs))]


def _sliding(eng, recs, p, window, hop, scopes, k):
    fr, qoff = _batch(recs)
    return eng.search_sliding_batch(fr, qoff, p, window, hop, k, scopes)


def _same(eng, recs, p, window, hop, scopes, k):
    got = _sliding(eng, recs, p, window, hop, scopes, k)
    assert got == _explicit(eng, recs, p, window, hop, scopes, k), (window, hop, k)
    assert [len(g) for g in got] == [W.nwin(len(f), window, hop) for f in recs]
    return got


def test_run_length_constant(tfp_lib):
    from tiresias_amd import _lib
    assert _lib.TFP_SLIDE_RUN == RUN


def test_goldens_every_case_k_1_and_4(engine, tfp_lib):
    scen, _ = R.load_cases()
    cases = W.load_sliding()
    W.no_empty_shell(cases)
    enrolled = None
    for name, qi, window, hop, ctx, wins in cases:
        s, q = scen[name], scen[name]["queries"][qi]
        if enrolled != name:
            S.enrol_scoped(engine, s)
            enrolled = name
        fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
        for k in (1, 4):
            for scopes in ([ctx], None) if ctx < 0 else ([ctx],):  # no context: TFP_SCOPE_ANY and scopes = NULL
                got = _sliding(engine, [fr], p, window, hop, scopes, k)[0]
                assert [R.pairs(r) for r in got] == [rows[:k] for rows in wins], (name, qi, window, hop, ctx, k)
    engine.index_clear()


def test_several_recordings_with_different_scopes_in_one_call(engine, tfp_lib, oracle):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    S.enrol_scoped(engine, s)
    by_p = {}
    for qi, q in enumerate(s["queries"]):
        if q["coefs"] in (1, 2) and len(q["q1"]) >= 12:
            by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
    done = set()
    for qis in by_p.values():
        q0 = s["queries"][qis[0]]
        if q0["coefs"] in done or q0["tol"] != q0["tol"]:
            continue
        done.add(q0["coefs"])
        p = _params(tfp_lib, q0)
        kinds = [0, 1, 2, ANY, S.UNUSED_SCOPE]
        recs = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in kinds]
        scopes = kinds * len(qis)
        window, hop = 4, 3
        got = _same(engine, recs, p, window, hop, scopes, 4)
        for r, rows in enumerate(got):
            q, x = s["queries"][qis[r // len(kinds)]], scopes[r]
            db = S.restrict(s, x) if x != ANY else (s["uuids"], s["clip"], s["m1"], s["m2"])
            for w, row in enumerate(rows):
                a = w * hop
                exp = R.brute_force(oracle, *db, q["q1"][a:a + window], q["q2"][a:a + window], q["coefs"], q["tol"], q["low"],
                                    q["high"], limit=4)
                assert R.pairs(row) == exp, (qis, r, w)
    assert done == {1, 2}
    engine.index_clear()


def _enrol_1030(engine):
    """1,030 clips of 3 rows (keys from 10..26), scope c % 2: the second column chunk is partial."""
    uuids = ["00000000-0000-4000-8000-%012d" % c for c in range(1030)]
    engine.index_clear()
    for c, u in enumerate(uuids):
        keys = sorted({10 + c % 7, 12 + c % 11, 14 + c % 13})
        engine.index_add(u, np.array([k * 1_000_000 + 500 for k in keys], np.int32), np.zeros(len(keys), np.int32))
    engine.index_set_scope(uuids, [c % 2 for c in range(1030)])
    return uuids


def _recording(rng, F, lo=10, hi=27):
    return R.frames_from_q([float(k) + 0.2 for k in rng.integers(lo, hi, F)], [0.0] * F)


def test_edge_shapes_against_the_explicit_windows(engine, tfp_lib):
    _enrol_1030(engine)
    rng = np.random.default_rng(94)
    p = tfp_lib.params(1, 0.001)
    shapes = []
    for hop in (1, 5, 7):  # window 5: 1, S - 1, S, S + 1 windows; window = F; window = F + 1; no frames
        shapes.append((5, hop, [5 + (n - 1) * hop for n in (1, RUN - 1, RUN, RUN + 1)] + [4, 0]))
    for hop in (1, 64, 66):
        shapes.append((64, hop, [63, 64, 65, 256, 257, 0]))
    for hop in (255, 256, 257):  # a slide staged in one tile, one full tile, a tile and one frame
        shapes.append((300, hop, [300 + 2 * hop + 3]))
    shapes.append((257, 1, [300]))
    for window, hop, Fs in shapes:
        recs = [_recording(rng, F) for F in Fs]
        scopes = [(0, 1, ANY)[i % 3] for i in range(len(Fs))]
        for k in (1, 8):
            got = _same(engine, recs, p, window, hop, scopes, k)
        assert any(len({r[0]["audio_uuid"] for r in rows if r}) > 1 for rows in got if rows) or window >= 257
        if window == 5:
            assert [len(g) for g in got] == [1, RUN - 1, RUN, RUN + 1, 0, 0]
    _same(engine, [_recording(rng, 40)], p, 5, 2, None, 3)
    assert _sliding(engine, [], p, 5, 1, None, 4) == []  # nrec = 0
    assert _sliding(engine, [_recording(rng, 0), _recording(rng, 3)], p, 5, 1, [0, 1], 4) == [[], []]
    engine.index_clear()
    assert _sliding(engine, [_recording(rng, 9)], p, 5, 1, None, 4) == [[[]] * 5]  # an empty index: five windows, no row


def test_ignored_and_null_frames_at_the_window_edges(engine, tfp_lib, oracle):
    uuids = _enrol_1030(engine)
    rng = np.random.default_rng(7)
    F, window = 90, 6
    q1 = [float(k) + 0.2 for k in rng.integers(10, 27, F)]
    for i in range(0, F, 5):   # -inf values: with window 6, hop 1 one is always entering or leaving
        q1[i] = -math.inf
    for i in range(2, F, 9):   # below / above the ignore thresholds (100 -> 20 dB, 250 -> 23.98 dB)
        q1[i] = 12.2 if i % 2 else 25.2
    fr = R.frames_from_q(q1, [0.0] * F)
    for low, high in ((100, 250), (-1, -1), (100, -1)):
        p = tfp_lib.params(1, 0.001, low, high)
        for hop in (1, 2, window, window + 2):
            got = _same(engine, [fr, fr], p, window, hop, [ANY, 1], 4)
        assert any(rows for rows in got[0])
    # the oracle's count for a few windows of the filtered search
    clip, m1 = [], []
    for c in range(1030):
        keys = sorted({10 + c % 7, 12 + c % 11, 14 + c % 13})
        clip += [c] * len(keys)
        m1 += [k * 1_000_000 + 500 for k in keys]
    p = tfp_lib.params(1, 0.001, 100, 250)
    got = _sliding(engine, [fr], p, window, 1, None, 8)[0]
    for w in (0, 1, 4, 5, 40, len(got) - 1):
        exp = R.brute_force(oracle, uuids, clip, m1, [0] * len(m1), q1[w:w + window], [0.0] * window, 1, 0.001, 100, 250,
                            limit=8)
        assert R.pairs(got[w]) == exp, w
    engine.index_clear()


def test_forced_general_form(tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    rng = np.random.default_rng(5)
    with tfp_lib.Engine(0) as eng:
        def stats():
            st = eng.slide_stats()
            return st["vote_batches"], st["general_batches"]

        # coefs = 2 at both tolerances, coefs = 1 at 0.45 (vote) and 9 (general)
        S.enrol_scoped(eng, s)
        recs = [R.frames_from_q(q["q1"], q["q2"]) for q in s["queries"] if q["coefs"] == 2 and len(q["q1"]) >= 12][:4]
        assert len(recs) >= 2
        hits = 0
        for coefs, tol, form in ((2, 0.001, 1), (2, 0.45, 1), (1, 0.45, 0), (1, 9.0, 1)):
            before = stats()
            got = _same(eng, recs, tfp_lib.params(coefs, tol), 4, 2, [ANY, 0, 1, 2][:len(recs)], 4)
            after = stats()
            assert (after[0] - before[0], after[1] - before[1]) == ((1, 0), (0, 1))[form], (coefs, tol)
            hits += sum(len(r) for rows in got for r in rows)
        assert hits > 20
        # one frame with a key outside the vote range in one recording of a batch
        uuids = _enrol_1030(eng)
        eng.index_add("ffffffff-0000-4000-8000-000000000000", np.array([600_000_100, 14_000_500], np.int32),
                      np.zeros(2, np.int32))
        eng.index_set_scope(["ffffffff-0000-4000-8000-000000000000"], [9])
        p = tfp_lib.params(1, 0.001)
        recs = [_recording(rng, 30) for _ in range(3)]
        before = stats()
        _same(eng, recs, p, 5, 1, None, 4)
        assert stats() == (before[0] + 1, before[1])
        recs[1]["q1"][17] = 600.0
        got = _same(eng, recs, p, 5, 1, [ANY, 9, 0], 4)
        assert stats() == (before[0] + 1, before[1] + 1)
        # the windows that hold frame 17 find the 600 dB row of the only clip in scope 9
        assert all(r and r[0]["audio_uuid"].startswith("ffffffff") for r in got[1][13:18])
        assert eng.slide_stats()["windows"] >= 2 * 3 * 26
        assert uuids


def test_index_delta(tfp_lib, monkeypatch):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    scen, _ = R.load_cases()
    name = max((n for n in scen if n.startswith("rand_")), key=lambda n: len(scen[n]["uuids"]))
    s = scen[name]
    nc = len(s["uuids"])
    clip = np.asarray(s["clip"], np.int64)
    m1 = np.asarray(s["m1"], np.int64).astype(np.int32)
    m2 = np.asarray(s["m2"], np.int64).astype(np.int32)
    with tfp_lib.Engine(0) as eng:
        for c in range(nc - 3):
            eng.index_add(s["uuids"][c], m1[clip == c], m2[clip == c])
        eng.index_set_scope(s["uuids"][:nc - 3], [c % 3 for c in range(nc - 3)])
        eng.index_commit()
        p = tfp_lib.params(1, 0.001)
        eng.search_ranked_batch(R.frames_from_q([24.3], [1.0]), [0, 1], p, 1)
        for c in range(nc - 3, nc):  # enrolled after the build
            eng.index_add(s["uuids"][c], m1[clip == c], m2[clip == c])
            eng.index_set_scope([s["uuids"][c]], [c % 3])
        # the recording: an old clip's own values, then a new clip's
        vals = [int(v) for c in (0, nc - 1) for v in m1[clip == c] if v != R.NULL]
        rec = R.frames_from_q([v / 1e6 for v in vals], [0.0] * len(vals))
        got = _sliding(eng, [rec, rec], p, 6, 2, [ANY, (nc - 1) % 3], 4)
        assert eng.index_delta_stats()[1] == 3 and eng.slide_stats()["vote_batches"] == 1  # served beside the index, no merge
        assert got == _explicit(eng, [rec, rec], p, 6, 2, [ANY, (nc - 1) % 3], 4)
        new = s["uuids"][nc - 1]
        for rows in got:  # the last window holds the new clip's own values only
            assert rows[-1] and rows[-1][0]["audio_uuid"] == new


def test_scope_and_output_contract(engine, tfp_lib):
    from tiresias_amd._lib import Candidate
    uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(5)]
    engine.index_clear()
    for c, u in enumerate(uuids):
        engine.index_add(u, np.array([(10 + c) * 1_000_000 + 500, 20_000_500], np.int32), np.zeros(2, np.int32))
    engine.index_set_scope(uuids, [1, 1, 2, 2, 2])
    rng = np.random.default_rng(3)
    fr = _recording(rng, 20, 10, 21)
    fr["q1"][3] = 20.2  # every clip has a row of key 20: the windows over frame 3 have all five
    p = tfp_lib.params(1, 0.001)
    L = tfp_lib.lib()

    def raw(window=4, hop=2, k=4, scope=ANY, cap=None, qoff=(0, 20), pp=p, scopes_null=False):
        cap = 9 if cap is None else cap
        out, cnt, nw = (Candidate * (max(cap, 1) * 32))(), (C.c_int32 * max(cap, 1))(), C.c_int64(-7)
        C.memset(out, 0xFF, C.sizeof(out))
        C.memset(cnt, 0xFF, C.sizeof(cnt))
        qo, sc = (C.c_int64 * len(qoff))(*qoff), (C.c_int32 * len(qoff))(*[scope] * len(qoff))
        rc = L.tfp_search_sliding_batch(engine.handle, fr.ctypes.data, qo, len(qoff) - 1, C.byref(pp), window, hop,
                                        None if scopes_null else sc, k, out, cnt, cap, C.byref(nw))
        return rc, out, list(cnt), nw.value

    # a scope no live clip has: every window is there, none has a row
    rc, out, cnt, nw = raw(scope=S.UNUSED_SCOPE)
    assert (rc, nw, cnt) == (0, 9, [0] * 9) and bytes(out)[:9 * 4 * C.sizeof(Candidate)] == bytes(9 * 4 * C.sizeof(Candidate))
    # k = 32 against 5 clips, output zeroed past counts
    rc, out, cnt, nw = raw(k=32)
    exp = _explicit(engine, [fr], p, 4, 2, None, 32)[0]
    assert (rc, nw) == (0, 9) and cnt == [len(r) for r in exp] and max(cnt) == 5
    one = C.sizeof(Candidate)
    for j in range(9):
        rows = out[j * 32:j * 32 + cnt[j]]
        assert [(c.uuid.decode(), c.match_count) for c in rows] == R.pairs(exp[j])
        assert bytes(out)[(j * 32 + cnt[j]) * one:(j + 1) * 32 * one] == bytes((32 - cnt[j]) * one)
    assert raw(k=32, scopes_null=True)[2] == cnt
    # too little room: *nwindows is set and nothing else written
    rc, out, cnt, nw = raw(cap=8)
    assert (rc, nw) == (TFP_E_CAPACITY, 9) and bytes(out) == b"\xff" * C.sizeof(out) and cnt == [-1] * 8
    rc, out, cnt, nw = raw(cap=0)
    assert (rc, nw) == (TFP_E_CAPACITY, 9)
    # arguments
    for kw in (dict(window=0), dict(window=-3), dict(hop=0), dict(hop=-1), dict(k=0), dict(k=33), dict(scope=-2),
               dict(pp=tfp_lib.params(3, 0.001)), dict(pp=tfp_lib.params(0, 0.001)), dict(qoff=(0, 12, 8))):
        rc, out, cnt, nw = raw(**kw)
        assert rc == TFP_E_ARG and bytes(out) == b"\xff" * C.sizeof(out), kw
    rc, out, cnt, nw = raw(window=21)  # window = F + 1
    assert (rc, nw) == (0, 0) and bytes(out) == b"\xff" * C.sizeof(out)
    v, g, w = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.tfp_slide_stats(engine.handle, None, None, None) == 0
    assert L.tfp_slide_stats(engine.handle, C.byref(v), C.byref(g), C.byref(w)) == 0 and v.value > 0 and w.value >= 9
    engine.index_clear()


def test_pcm_form(engine, tfp_lib):
    n = 8000 * 4
    pcm = tfp_lib.synth_pcm(0x7153A1, range(3), n)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(4) * n)
    nf = len(fr) // 3
    uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(3)]
    engine.index_clear()
    for c in range(3):
        engine.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    engine.index_set_scope(uuids, [3, 4, 3])
    noise = tfp_lib.synth_pcm(0xBEEF, range(3), 6000)
    # three recordings of different lengths: noise, an excerpt of an enrolled clip from a hop boundary, noise
    recs = [np.concatenate([noise[i][:256 * (3 + i)], pcm[i][256 * 20:256 * 20 + ln], noise[i][:1000 + 300 * i]])
            for i, ln in enumerate((12000, 7000 + 77, 3000))]
    flat = np.concatenate(recs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    rfr = engine.fingerprint_batch(flat, off)
    foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(len(r)) for r in recs])])
    assert len(rfr) == foff[-1] and len(set(np.diff(foff))) == 3
    window, hop = 12, 5
    found = 0
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        for scopes in (None, [3, 4, ANY], [4, 3, 0]):
            got = engine.search_sliding_pcm_batch(flat, off, p, window, hop, 3, scopes)
            assert got == engine.search_sliding_batch(rfr, foff, p, window, hop, 3, scopes), (p.coefs, scopes)
            assert got == _explicit(engine, [rfr[foff[i]:foff[i + 1]] for i in range(3)], p, window, hop, scopes, 3)
            found += sum(bool(r) for rows in got for r in rows)
        # window 0 is the ranked PCM search of the first window * 256 samples
        heads = [r[:window * 256] for r in recs]
        first = engine.search_ranked_pcm_batch(np.concatenate(heads), np.arange(4) * window * 256, p, 3)
        got = engine.search_sliding_pcm_batch(flat, off, p, window, hop, 3)
        assert [rows[0] for rows in got] == first
    assert found > 4  # windows with rows
    engine.index_clear()


def test_group_of_three_equals_one_engine(engine, tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    g = tfp_lib.Group([0, 0, 0])
    try:
        S.enrol_scoped(engine, s)
        S.enrol_scoped(g, s)
        n = 0
        for coefs in (1, 2):
            qs = [q for q in s["queries"] if q["coefs"] == coefs and len(q["q1"]) >= 12 and q["tol"] == q["tol"]][:5]
            p = _params(tfp_lib, qs[0])
            recs = [R.frames_from_q(q["q1"], q["q2"]) for q in qs]
            fr, qoff = _batch(recs)
            for scopes in (None, [0, 1, 2, ANY, S.UNUSED_SCOPE][:len(recs)]):
                got = g.search_sliding_batch(fr, qoff, p, 4, 3, 4, scopes)
                want = engine.search_sliding_batch(fr, qoff, p, 4, 3, 4, scopes)
                assert [[R.pairs(r) for r in rows] for rows in got] == [[R.pairs(r) for r in rows] for rows in want]
                assert all(0 <= c["clip_id"] < 3 for rows in got for r in rows for c in r)  # clip_id is the shard
                n += sum(len(r) for rows in got for r in rows)
        assert n > 50
        assert g.search_sliding_batch(np.zeros(0, R.FRAME_DTYPE), [0], tfp_lib.params(1, 0.001), 4, 1, 4) == []
    finally:
        g.close()
        engine.index_clear()
