"""Sliding aligned search (tfp_align_sliding_batch, tfp_search_sliding_aligned*, csrc/tfp_slide_align.hip):
for every window of a recording and every row of its result, the alignment of that window's frames
alone with the row's clip, against the SQLite-derived fixture tests/golden/sliding_aligned_cases.json,
align_util.brute_force (the goldens' further rows, the occurrence in the PCM test), its arithmetic over one
hit matrix per clip (slide_align_util.four_of_hits: the synthetic shapes' every window), and align_batch
(unchanged code) called on the windows cut out on the host.

The slid kernel takes 256 run-relative diagonals per block and stages up to 256 leaving and 256
entering frames per step; the synthetic shapes below cross the band edges (clips of 255, 256, 257 and
300 rows under a 700-frame recording), put ties on every diagonal, and take both forms of the run
rule: slid where 2 * hop < window, direct elsewhere and for single-entry runs."""
import ctypes as C
import math

import numpy as np
import pytest

import align_util as A
import ranked_util as R
import scoped_util as S
import slide_align_util as SA
import sliding_util as W

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_NOENT, TFP_E_CAPACITY = -1, -4, -5
ANY = -1
ZERO = SA.ZERO
SHAPES = [(94, 1), (94, 8), (300, 7), (16, 7), (16, 8), (1, 1), (700, 1)]
SLID = {(94, 1), (94, 8), (300, 7), (16, 7)}  # 2 * hop < window
FORMS = ((1, 0.001), (2, 0.45))  # (coefs, tolerance): the sliding search's vote form and its general form
F_REC, OCC = 700, (123, 500)
CLIP_KEYS = ("aligned_count", "offset", "first_frame", "last_frame")


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _batch(frames):
    return (np.concatenate(frames) if frames else np.zeros(0, R.FRAME_DTYPE),
            np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64))


def _plain(rows):
    """The rows without their alignment: what search_sliding_batch returns."""
    return [{k: v for k, v in r.items() if k not in CLIP_KEYS} for r in rows]


def _forms(entries, window, hop):
    """(slid, direct) entries by the run rule: entries = {(recording, clip): sorted windows}."""
    slid = direct = 0
    for ws in entries.values():
        runs, cur = [], [ws[0]]
        for w in ws[1:]:
            if (w - cur[-1]) * hop >= window:
                runs.append(cur)
                cur = []
            cur.append(w)
        runs.append(cur)
        for run in runs:
            if len(run) == 1 or 2 * hop >= window:
                direct += len(run)
            else:
                slid += len(run)
    return slid, direct


def _entries_of(got):
    ent = {}
    for r, wins in enumerate(got):
        for w, rows in enumerate(wins):
            for row in rows:
                ent.setdefault((r, row["audio_uuid"]), []).append(w)
    return ent


def _moved(eng, before):
    st = eng.slide_align_stats()
    return st["batches"] - before["batches"], st["slid_entries"] - before["slid_entries"], \
        st["direct_entries"] - before["direct_entries"]


def test_goldens_every_case_k_1_and_4(engine, tfp_lib, oracle):
    scen, _ = R.load_cases()
    enrolled, fixture_rows, brute_rows = None, 0, 0
    for name, qi, window, hop, ctx, wins, _added in SA.load_sliding_aligned():
        s, q = scen[name], scen[name]["queries"][qi]
        col = {u: c for c, u in enumerate(s["uuids"])}
        if enrolled != name:
            S.enrol_scoped(engine, s)
            enrolled = name
        fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
        for k in (1, 4):
            for scopes in ([ctx], None) if ctx < 0 else ([ctx],):
                got = engine.search_sliding_aligned_batch(fr, [0, len(fr)], p, window, hop, k, scopes)[0]
                want = engine.search_sliding_batch(fr, [0, len(fr)], p, window, hop, k, scopes)[0]
                assert [_plain(r) for r in got] == want, (name, qi, window, hop, ctx, k)  # out and counts as the sliding search's
                for w, rows in enumerate(got):
                    a = w * hop
                    for i, row in enumerate(rows):
                        if i < SA.ROWS:
                            assert (row["audio_uuid"], row["match_count"]) + A.four(row) == wins[w][i], (name, qi, w, i, k)
                            fixture_rows += 1
                        elif scopes is not None:
                            m1, m2 = A.clip_rows(s, col[row["audio_uuid"]])
                            exp = A.brute_force(oracle, m1, m2, q["q1"][a:a + window], q["q2"][a:a + window], q["coefs"],
                                                q["tol"], q["low"], q["high"])
                            assert A.four(row) == exp, (name, qi, w, i, k)
                            brute_rows += 1
    engine.index_clear()
    assert fixture_rows > 1500 and brute_rows > 100


def test_composed_definition_several_recordings_and_scopes(engine, tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    S.enrol_scoped(engine, s)
    done = set()
    for coefs in (1, 2):
        qs = [q for q in s["queries"] if q["coefs"] == coefs and len(q["q1"]) >= 12 and q["tol"] == q["tol"]]
        q0 = qs[0]
        qs = [q for q in qs if (repr(q["tol"]), q["low"], q["high"]) == (repr(q0["tol"]), q0["low"], q0["high"])][:4]
        p = _params(tfp_lib, q0)
        scopes = [0, 1, 2, ANY, S.UNUSED_SCOPE]
        recs = [R.frames_from_q(q["q1"], q["q2"]) for q in qs for _ in scopes]
        scopes = scopes * len(qs)
        fr, qoff = _batch(recs)
        for window, hop, k in ((6, 1, 4), (4, 3, 4), (5, 2, 2)):
            before = engine.slide_align_stats()
            got = engine.search_sliding_aligned_batch(fr, qoff, p, window, hop, k, scopes)
            assert [[_plain(r) for r in wins] for wins in got] == engine.search_sliding_batch(fr, qoff, p, window, hop, k, scopes)
            b, slid, direct = _moved(engine, before)
            assert (b, slid, direct) == (1,) + _forms(_entries_of(got), window, hop)
            # the definition: every window cut out on the host, align_batch with the sliding rows' clip ids
            cuts, ids = [], []
            for rec, wins in zip(recs, got):
                for w, rows in enumerate(wins):
                    cuts.append(rec[w * hop:w * hop + window])
                    ids.append([r["clip_id"] for r in rows] + [-1] * (k - len(rows)))
            cfr, coff = _batch(cuts)
            exp = engine.align_batch(cfr, coff, p, np.array(ids, np.int32), k)
            j = 0
            for wins in got:
                for rows in wins:
                    assert [A.four(r) for r in rows] == [A.four(e) for e in exp[j][:len(rows)]], (coefs, window, hop, j)
                    j += 1
            assert j == len(cuts) > 20
            done.add((coefs, slid > 0, direct > 0))
    assert {d[0] for d in done} == {1, 2} and any(d[1] for d in done) and any(d[2] for d in done)
    engine.index_clear()


# ---- the synthetic index: band and tile crossings, ties, NULL rows, two occurrences -----------------------
def _uuid(c):
    return "00000000-0000-4000-8000-%012d" % c


def _synthetic():
    """(clips [(m1, m2)], q1, q2): clips of 1, 255, 256, 257 rows, an all-equal clip, a clip with NULL rows and
    clip-300 (the last: the greatest uuid, so row 0 where the counts tie), max1 over 6 key values and max2 over 3;
    a 700-frame recording of the same values holding clip-300's rows from frame 123 and again from frame 500."""
    rng = np.random.default_rng(0x51DE)
    clips = []
    for n in (1, 255, 256, 257, 120, 200, 300):
        m1 = rng.integers(20, 26, n).astype(np.int64) * 1_000_000 + 500
        m2 = rng.integers(5, 8, n).astype(np.int64) * 1_000_000
        clips.append((m1, m2))
    clips[4] = (np.full(120, 22_000_500, np.int64), np.full(120, 6_000_000, np.int64))  # every diagonal ties
    clips[5][0][[0, 1, 57, 128, 199]] = R.NULL
    clips[5][1][[3, 57, 198]] = R.NULL
    k1, k2 = rng.integers(20, 26, F_REC), rng.integers(5, 8, F_REC)
    m1, m2 = clips[6]
    for at in OCC:
        n = min(300, F_REC - at)
        k1[at:at + n], k2[at:at + n] = m1[:n] // 1_000_000, m2[:n] // 1_000_000
    return clips, [float(v) + 0.2 for v in k1], [float(v) for v in k2]


@pytest.fixture(scope="module")
def synth(oracle):
    """The synthetic shapes' reference, computed once: per (coefs, tolerance) and (window, hop), per clip the
    alignment of every window. The oracle for every window is slide_align_util.four_of_hits over one
    align_util.hit_matrix of the whole recording (the oracle's frame boxes, one pass per clip), independent of the
    code under test; align_util.brute_force itself is called on five windows per form below, to show that the two
    give the same four integers."""
    clips, q1, q2 = _synthetic()
    ref = {}
    for coefs, tol in FORMS:
        hits = [A.hit_matrix(oracle, m1, m2, q1, q2, coefs, tol, -1, -1) for m1, m2 in clips]
        for window, hop in SHAPES:
            ref[(coefs, window, hop)] = [SA.window_fours(h, window, hop) for h in hits]
    # five windows per form through align_util.brute_force itself
    for coefs, tol in FORMS:
        for (window, hop), w, c in (((94, 8), 3, 6), ((94, 8), 50, 1), ((300, 7), 20, 3), ((16, 7), 70, 4), ((700, 1), 0, 5)):
            a = w * hop
            assert ref[(coefs, window, hop)][c][w] == A.brute_force(oracle, *clips[c], q1[a:a + window], q2[a:a + window],
                                                                     coefs, tol)
    return clips, R.frames_from_q(q1, q2), ref


def _enrol_synth(eng, clips):
    eng.index_clear()
    for c, (m1, m2) in enumerate(clips):  # (after a clear the clip ids count from 0 in this order)
        eng.index_add(_uuid(c), m1.astype(np.int32), m2.astype(np.int32))


def test_band_and_tile_crossings_through_the_search_form(engine, tfp_lib, synth):
    clips, rec, ref = synth
    _enrol_synth(engine, clips)
    col = {_uuid(c): c for c in range(len(clips))}
    tied = 0
    for coefs, tol in FORMS:
        p = tfp_lib.params(coefs, tol)
        for window, hop in SHAPES:
            before = engine.slide_align_stats()
            got = engine.search_sliding_aligned_batch(rec, [0, F_REC], p, window, hop, 4)[0]
            assert len(got) == W.nwin(F_REC, window, hop)
            assert [_plain(r) for r in got] == engine.search_sliding_batch(rec, [0, F_REC], p, window, hop, 4)[0]
            for w, rows in enumerate(got):
                for row in rows:
                    assert A.four(row) == ref[(coefs, window, hop)][col[row["audio_uuid"]]][w], (coefs, window, hop, w, row)
            b, slid, direct = _moved(engine, before)
            assert (b, slid, direct) == (1,) + _forms(_entries_of([got]), window, hop), (window, hop)
            assert (slid > 0) == ((window, hop) in SLID) and (direct > 0 or (window, hop) in SLID), (window, hop, slid, direct)
            # the occurrences of clip-300: row 0 with every frame on one diagonal, which names the occurrence
            for at in OCC:
                inside = [w for w in range(len(got)) if at <= w * hop and w * hop + window <= min(at + 300, F_REC)]
                assert inside or window > 200
                for w in inside:
                    top = got[w][0]
                    assert top["audio_uuid"] == _uuid(6) and top["aligned_count"] == window == top["match_count"]
                    assert (top["first_frame"], top["last_frame"]) == (0, window - 1)
                    # (one frame's value recurs in the clip and the smallest offset wins: window 1 names no occurrence)
                    assert w * hop - top["offset"] == at if window > 1 else w * hop - top["offset"] >= at
            tied += sum(r["audio_uuid"] == _uuid(4) for rows in got for r in rows)
    assert tied > 100  # the all-equal clip is among the rows: every diagonal of it ties and the smallest wins
    engine.index_clear()


def test_call_paths_through_the_primitive(engine, tfp_lib, synth):
    clips, rec, ref = synth
    _enrol_synth(engine, clips)
    k = 3
    for coefs, tol in FORMS:
        p = tfp_lib.params(coefs, tol)
        for window, hop in SHAPES:
            nw = W.nwin(F_REC, window, hop)
            ids = np.full((nw, k), -1, np.int32)
            for w in range(nw):
                if w <= 5 or w >= 40:
                    ids[w, 0] = 6        # windows 0-5 and again from 40: two runs wherever a run holds fewer than 35 windows
                ids[w, 1] = w % 5        # clips 0-4 each fifth window: runs with windows no entry needs
            if nw > 7:
                ids[7, 2] = 5            # one window only: a single-entry run
            ent = {}
            for w in range(nw):
                for c in ids[w]:
                    if c >= 0:
                        ent.setdefault((0, int(c)), []).append(w)
            before = engine.slide_align_stats()
            got = engine.align_sliding_batch(rec, [0, F_REC], p, window, hop, ids, k)[0]
            b, slid, direct = _moved(engine, before)
            assert (b, slid, direct) == (1,) + _forms(ent, window, hop), (window, hop)
            assert (slid > 0) == ((window, hop) in SLID) and direct >= 1, (window, hop, slid, direct)
            for w in range(nw):
                for i in range(k):
                    exp = ref[(coefs, window, hop)][ids[w, i]][w] if ids[w, i] >= 0 else ZERO
                    assert A.four(got[w][i]) == exp, (coefs, window, hop, w, i)
    # the run rule on such a grid: windows 0-5 and 40-49 are two runs at (16, 7) and one at (94, 1); one window alone is direct
    assert _forms({(0, 6): list(range(6)) + list(range(40, 50)), (0, 5): [7]}, 16, 7) == (16, 1)
    assert _forms({(0, 6): list(range(6)) + list(range(40, 50)), (0, 5): [7]}, 94, 1) == (16, 1)
    assert _forms({(0, 6): list(range(6)) + list(range(40, 50)), (0, 5): [7]}, 16, 8) == (0, 17)
    # the same clip twice in one window: both entries get its alignment
    p = tfp_lib.params(1, 0.001)
    nw = W.nwin(F_REC, 94, 8)
    ids = np.full((nw, 2), 3, np.int32)
    got = engine.align_sliding_batch(rec, [0, F_REC], p, 94, 8, ids, 2)[0]
    assert all(A.four(got[w][i]) == ref[(1, 94, 8)][3][w] for w in range(nw) for i in range(2))
    engine.index_clear()


def test_ignored_and_null_frames_enter_and_leave_the_slid_sums(engine, tfp_lib, oracle, synth):
    clips, _, _ = synth
    _enrol_synth(engine, clips)
    rng = np.random.default_rng(7)
    F, window = 120, 6
    q1 = [float(k) + 0.2 for k in rng.integers(20, 26, F)]
    q2 = [float(k) for k in rng.integers(5, 8, F)]
    for i in range(0, F, 5):   # NULL values: with window 6, hop 1 one is always at a window's first or last frame
        q1[i] = -math.inf
    for i in range(3, F, 11):
        q2[i] = -math.inf
    for i in range(2, F, 9):   # below / above the ignore thresholds (150 -> 21.76 dB, 250 -> 23.98 dB)
        q1[i] = 20.2 if i % 2 else 25.2
    fr = R.frames_from_q(q1, q2)
    ids_all = np.arange(len(clips), dtype=np.int32)
    changed = 0
    for coefs, tol in FORMS:
        for low, high in ((150, 250), (-1, -1), (150, -1)):
            p = tfp_lib.params(coefs, tol, low, high)
            hits = [A.hit_matrix(oracle, m1, m2, q1, q2, coefs, tol, low, high) for m1, m2 in clips]
            for hop in (1, 2, 3):
                nw = W.nwin(F, window, hop)
                before = engine.slide_align_stats()
                got = engine.align_sliding_batch(fr, [0, F], p, window, hop, np.tile(ids_all, nw), len(clips))[0]
                assert _moved(engine, before) == ((1, nw * len(clips), 0) if 2 * hop < window else (1, 0, nw * len(clips)))
                for c, h in enumerate(hits):
                    exp = SA.window_fours(h, window, hop)
                    assert [A.four(got[w][c]) for w in range(nw)] == exp, (coefs, low, high, hop, c)
            changed += hits[1].sum() != A.hit_matrix(oracle, *clips[1], q1, q2, coefs, tol, -1, -1).sum()
            got = engine.search_sliding_aligned_batch(fr, [0, F], p, window, 1, 3)[0]
            for w, rows in enumerate(got):
                for row in rows:
                    c = int(row["audio_uuid"][-3:])
                    assert A.four(row) == SA.four_of_hits(hits[c][w:w + window])
    assert changed >= 3  # the filters do change the hits
    engine.index_clear()


def test_contract(engine, tfp_lib, synth):
    from tiresias_amd._lib import Alignment, Candidate
    clips, rec, ref = synth
    _enrol_synth(engine, clips)
    L = tfp_lib.lib()
    p = tfp_lib.params(1, 0.001)
    fr = rec[:40]

    def raw_search(window=8, hop=4, k=4, scope=ANY, cap=9, qoff=(0, 40), pp=p):
        out, cnt = (Candidate * (max(cap, 1) * 32))(), (C.c_int32 * max(cap, 1))()
        al, nw = (Alignment * (max(cap, 1) * 32))(), C.c_int64(-7)
        for buf in (out, cnt, al):
            C.memset(buf, 0xFF, C.sizeof(buf))
        qo, sc = (C.c_int64 * len(qoff))(*qoff), (C.c_int32 * len(qoff))(*[scope] * len(qoff))
        rc = L.tfp_search_sliding_aligned_batch(engine.handle, fr.ctypes.data, qo, len(qoff) - 1, C.byref(pp), window, hop,
                                                sc, k, out, cnt, al, cap, C.byref(nw))
        untouched = all(bytes(b) == b"\xff" * C.sizeof(b) for b in (out, cnt, al))
        return rc, nw.value, untouched, out, cnt, al

    def raw_align(window=8, hop=4, k=2, cap=9, qoff=(0, 40), pp=p, ids=None):
        idv = np.full(max(cap, 1) * 32, 6, np.int32) if ids is None else np.asarray(ids, np.int32)
        al, nw = (Alignment * (max(cap, 1) * 32))(), C.c_int64(-7)
        C.memset(al, 0xFF, C.sizeof(al))
        qo = (C.c_int64 * len(qoff))(*qoff)
        rc = L.tfp_align_sliding_batch(engine.handle, fr.ctypes.data, qo, len(qoff) - 1, C.byref(pp), window, hop,
                                       idv.ctypes.data, k, al, cap, C.byref(nw))
        return rc, nw.value, bytes(al) == b"\xff" * C.sizeof(al), al

    # enough room: 9 windows, entries past counts zeroed
    rc, nw, untouched, out, cnt, al = raw_search(k=32)
    assert (rc, nw) == (0, 9) and not untouched and 1 <= max(cnt[:9]) <= len(clips)
    one = C.sizeof(Alignment)
    for j in range(9):
        assert all(al[j * 32 + i].aligned_count >= 1 for i in range(cnt[j]))
        assert bytes(al)[(j * 32 + cnt[j]) * one:(j + 1) * 32 * one] == bytes((32 - cnt[j]) * one)
    # too little room: *nwindows is set and nothing else written
    for cap in (8, 0):
        assert raw_search(cap=cap)[:3] == (TFP_E_CAPACITY, 9, True)
        assert raw_align(cap=cap)[:3] == (TFP_E_CAPACITY, 9, True)
    # each argument case of the sliding call
    for kw in (dict(window=0), dict(window=-3), dict(hop=0), dict(hop=-1), dict(k=0), dict(k=33),
               dict(pp=tfp_lib.params(3, 0.001)), dict(pp=tfp_lib.params(0, 0.001)), dict(qoff=(0, 12, 8))):
        assert raw_search(**kw)[0] == TFP_E_ARG and raw_search(**kw)[2], kw
        assert raw_align(**kw)[0] == TFP_E_ARG and raw_align(**kw)[2], kw
    assert raw_search(scope=-2)[0] == TFP_E_ARG and raw_search(scope=-2)[2]
    # a bad id, in any position; -1 is no id
    for bad in (len(clips), -2, 1 << 30):
        ids = np.full(9 * 2, -1, np.int32)
        ids[11] = bad
        assert raw_align(ids=ids)[0] == TFP_E_NOENT, bad
    rc, nw, untouched, al = raw_align(ids=np.full(18, -1, np.int32))
    assert (rc, nw) == (0, 9) and bytes(al)[:18 * one] == bytes(18 * one)
    engine.index_remove(_uuid(2))
    ids = np.full(18, -1, np.int32)
    ids[4] = 2
    assert raw_align(ids=ids)[0] == TFP_E_NOENT
    # a recording shorter than the window: no window, nothing launched, nothing written
    assert engine.search_sliding_aligned_batch(fr, [0, 5, 5, 40], p, 8, 4, 2)[:2] == [[], []]
    before = engine.slide_align_stats()
    assert raw_search(window=41)[:3] == (0, 0, True) and raw_align(window=41)[:3] == (0, 0, True)
    # an empty index: the windows are there, no row, nothing launched
    engine.index_clear()
    assert engine.search_sliding_aligned_batch(fr, [0, 40], p, 8, 4, 2) == [[[]] * 9]
    rc, nw, untouched, out, cnt, al = raw_search()
    assert (rc, nw, list(cnt)) == (0, 9, [0] * 9) and bytes(al)[:9 * 4 * one] == bytes(9 * 4 * one)
    assert _moved(engine, before) == (0, 0, 0)
    b, s, d = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.tfp_slide_align_stats(engine.handle, None, None, None) == 0
    assert L.tfp_slide_align_stats(engine.handle, C.byref(b), C.byref(s), C.byref(d)) == 0 and min(b.value, s.value, d.value) >= 0


def test_index_delta_and_staging_compaction(tfp_lib, monkeypatch, synth, oracle):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    clips, rec, ref = synth
    p = tfp_lib.params(1, 0.001)
    with tfp_lib.Engine(0) as eng:
        for c in range(5):
            eng.index_add(_uuid(c), clips[c][0].astype(np.int32), clips[c][1].astype(np.int32))
        eng.index_commit()
        eng.search_ranked_batch(R.frames_from_q([24.3], [1.0]), [0, 1], p, 1)
        for c in (5, 6):  # enrolled after the build
            eng.index_add(_uuid(c), clips[c][0].astype(np.int32), clips[c][1].astype(np.int32))
        window, hop = 94, 8
        got = eng.search_sliding_aligned_batch(rec, [0, F_REC], p, window, hop, 4)[0]
        assert eng.index_delta_stats()[1] == 2  # served beside the index, no merge
        col = {_uuid(c): c for c in range(len(clips))}
        for w, rows in enumerate(got):
            assert rows[0]["audio_uuid"] == _uuid(6) or not (123 <= w * hop and w * hop + window <= 423)
            for row in rows:
                assert A.four(row) == ref[(1, window, hop)][col[row["audio_uuid"]]][w], (w, row)
        assert any(r["audio_uuid"] in (_uuid(5), _uuid(6)) for rows in got for r in rows)
        # clips removed and added between two calls: the staging arrays are compacted, the rows the same
        eng.index_remove(_uuid(1))
        eng.index_remove(_uuid(3))
        eng.index_add(_uuid(1), clips[1][0].astype(np.int32), clips[1][1].astype(np.int32))
        eng.index_add(_uuid(3), clips[3][0].astype(np.int32), clips[3][1].astype(np.int32))
        eng.index_commit()
        again = eng.search_sliding_aligned_batch(rec, [0, F_REC], p, window, hop, 4)[0]
        strip = lambda wins: [[{k: v for k, v in r.items() if k != "clip_id"} for r in rows] for rows in wins]  # noqa: E731
        assert strip(again) == strip(got)


def test_pcm_form_equals_the_frames_form(engine, tfp_lib, oracle):
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
    rows_seen = 0
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        for window, hop in ((12, 5), (12, 7)):
            for scopes in (None, [3, 4, ANY]):
                got = engine.search_sliding_aligned_pcm_batch(flat, off, p, window, hop, 3, scopes)
                assert got == engine.search_sliding_aligned_batch(rfr, foff, p, window, hop, 3, scopes), (p.coefs, window, hop)
                assert [[_plain(r) for r in wins] for wins in got] == engine.search_sliding_pcm_batch(flat, off, p, window, hop,
                                                                                                       3, scopes)
                rows_seen += sum(r["aligned_count"] >= 1 for wins in got for rows in wins for r in rows)
    assert rows_seen > 4  # windows with rows
    # an occurrence: a 8 s clip of noise whose level moves from hop to hop (which moves max1's truncated key as far
    # as 10 log10 |c0| lets it), and a recording of 50 frames of noise, the clip's frames 40-226 and noise again. A
    # frame hits its own stored row when max1 lies within the tolerance of its truncated key (fp_handler.c:290), so
    # at tolerance 0.999 every frame does, and a window inside the excerpt, past its first frame (whose analysis
    # window still sees the noise), has all its frames on the occurrence's diagonal; the oracle's fingerprints and
    # the brute force say that no other diagonal of any such window reaches the count. So every window names the
    # occurrence: recording frame 50 is clip frame 40, w * hop - offset = 10
    rng = np.random.default_rng(0x7153A1)
    gain = np.repeat(10 ** rng.uniform(-2.7, 0, 250), 256)
    clip = np.clip(rng.normal(size=250 * 256) * 7000 * gain, -32767, 32767).astype(np.int16)
    cfr = engine.fingerprint_batch(clip, [0, len(clip)])
    engine.index_add(_uuid(3), cfr["m1"], cfr["m2"])
    far = tfp_lib.synth_pcm(0xBEEF, range(2), 256 * 60)
    rec = np.concatenate([far[0][:256 * 50], clip[256 * 40:256 * 227], far[1][:256 * 45 + 100]])
    window, hop, p = 48, 6, tfp_lib.params(1, 0.999)
    got = engine.search_sliding_aligned_pcm_batch(rec, [0, len(rec)], p, window, hop, 4)[0]
    inside = [w for w in range(len(got)) if 50 + 1 <= w * hop and w * hop + window <= 50 + 187]
    assert len(inside) >= 20
    micro, qdb = oracle.fingerprint(clip)[2], oracle.fingerprint(rec)[1]
    for w in inside:
        exp, _, tie = A.brute_force(oracle, micro[:, 0], micro[:, 1], list(qdb[w * hop:w * hop + window, 0]),
                                    list(qdb[w * hop:w * hop + window, 1]), 1, 0.999, more=True)
        assert exp == (window, w * hop - 10, 0, window - 1) and not tie, (w, exp, tie)
        row = next(r for r in got[w] if r["audio_uuid"] == _uuid(3))
        assert A.four(row) == exp and row["match_count"] == window and w * hop - row["offset"] == 10, (w, row)
    engine.index_clear()


def test_group_of_three_equals_one_engine(engine, tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    g = tfp_lib.Group([0, 0, 0])
    try:
        S.enrol_scoped(engine, s)
        S.enrol_scoped(g, s)
        n = mixed = 0
        for coefs in (1, 2):
            qs = [q for q in s["queries"] if q["coefs"] == coefs and len(q["q1"]) >= 12 and q["tol"] == q["tol"]][:5]
            p = _params(tfp_lib, qs[0])
            fr, qoff = _batch([R.frames_from_q(q["q1"], q["q2"]) for q in qs])
            for window, hop in ((6, 1), (4, 3)):
                for scopes in (None, [0, 1, 2, ANY, S.UNUSED_SCOPE][:len(qs)]):
                    got = g.search_sliding_aligned_batch(fr, qoff, p, window, hop, 4, scopes)
                    want = engine.search_sliding_aligned_batch(fr, qoff, p, window, hop, 4, scopes)
                    drop = lambda x: [[[{k: v for k, v in r.items() if k != "clip_id"} for r in rows] for rows in wins]  # noqa: E731
                                      for wins in x]
                    assert drop(got) == drop(want), (coefs, window, hop, scopes)
                    assert all(0 <= r["clip_id"] < 3 for wins in got for rows in wins for r in rows)  # clip_id is the shard
                    n += sum(len(rows) for wins in got for rows in wins)
                    mixed += sum(len({r["clip_id"] for r in rows}) > 1 for wins in got for rows in wins)
        assert n > 100 and mixed > 0  # windows whose rows come from two shards
        assert g.search_sliding_aligned_batch(np.zeros(0, R.FRAME_DTYPE), [0], tfp_lib.params(1, 0.001), 4, 1, 4) == []
    finally:
        g.close()
        engine.index_clear()
