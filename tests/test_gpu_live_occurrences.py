"""The log of a live call (tfp_live_occurrences, tfp_live_tracks, tfp_live_occurrence_stats; csrc/tfp_live_trace.hip
live_trace_kernel): after every call the occurrences, the dropped counts, every channel's list with its traces
and the (track, frame) pairs folded equal the composition of entry points that have parity tests of their own
(live_occurrence_util.Ref: tfp_live_frames, tfp_search_scoped_batch, tfp_align_batch, tfp_trace_batch and the
header's offer and suppression rules). Integers throughout: every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import live_occurrence_util as LO
import live_window_util as W

pytestmark = pytest.mark.gpu

T = LO.T
INT32_MAX = 2 ** 31 - 1
NCH, WINDOW, K = 3, 48, 3
FRAMES = 180  # every call's length
GAP, HITS = 5, 10
A, B = 2, 3   # channel 0 plays clip A from frame 20 and clip B from frame 99
SCOPES = [0, 2, 1]  # each channel's own context (LO.SCOPE_OF): the clips it plays and one or two more


@pytest.fixture(scope="module")
def world(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    old = os.environ.get("TFP_INDEX_DELTA")
    os.environ["TFP_INDEX_DELTA"] = "1"  # the index delta at this DB size too
    try:
        eng = tfp_lib.Engine(0)
    finally:
        if old is None:
            del os.environ["TFP_INDEX_DELTA"]
        else:
            os.environ["TFP_INDEX_DELTA"] = old
    db = LO.build_db(tfp_lib, eng)
    yield eng, db, calls(tfp_lib, db)
    eng.close()


def calls(tfp, db):
    """Three calls of FRAMES frames. 0: noise, clip A, a gap of noise, clip B, noise. 1: joined inside clip 5
    (its frame 30: s = -30), silence, then the delta's clip, still playing when the call ends. 2: silence,
    clip 1, noise, clip 1 again, silence."""
    pcm, z = db["pcm"], lambda f: np.zeros(f * 256, np.int16)
    c0 = np.concatenate([LO.noise(tfp, 20 * 256), pcm[A], LO.noise(tfp, 15 * 256, 901), pcm[B], LO.noise(tfp, 6 * 256, 902)])
    c1 = np.concatenate([pcm[5][30 * 256:], z(10), pcm[LO.LATE][:99 * 256]])
    c2 = np.concatenate([z(12), pcm[1], LO.noise(tfp, 20 * 256, 903), pcm[1], z(34)])
    src = np.stack([c0, c1, c2])
    assert src.shape == (NCH, FRAMES * 256)
    return src


class Call:
    def __init__(self, tfp, world, nch=NCH):
        self.tfp = tfp
        self.eng, self.db, self.src = world
        self.lv = tfp.Live(self.eng, nch, FRAMES * 256)
        self.ref = LO.Ref(tfp, self.eng, self.lv, self.db)
        self.hist = [np.zeros(0, np.int16) for _ in range(nch)]
        self.at = 0
        self.args = dict(p=tfp.params(1, 0.45), scopes=list(SCOPES), k=K, window=WINDOW, max_gap=GAP, min_hits=HITS, max_tracks=64)

    def push(self, n):
        W.push_all(self.lv, self.hist, self.src[:, self.at:self.at + n])
        self.at += n

    def check(self, where=None):
        return self.ref.call(where=(where, self.at), **self.args)

    def ticks(self, n, size=T, where=None):
        for _ in range(n):
            self.push(size)
            got = self.check(where)
        return got

    def close(self):
        self.lv.close()


def _entry(occ, uuid, s):
    hit = [o for o in occ if o["audio_uuid"] == uuid and o["clip_start_frame"] == s]
    assert len(hit) == 1, (uuid, s, occ)
    return {q: hit[0][q] for q in ("first_frame", "last_frame", "hits", "diagonal_hits", "overlap")}


def test_every_tick_and_the_finished_call(tfp_lib, world):
    """Ticks of 160 samples, checked after every tick, every channel searching its own context: silence or
    noise, a clip, a gap, another clip; a call joined mid-clip (s < 0); a clip of the index delta still playing
    at the last tick (its span reaches past F); one clip played twice. At the end the log names the played
    clips at their true starts, A at 20 and B at 99 among them, with the extents the batch form gives on the
    finished call's frames."""
    eng, db, _ = world
    c = Call(tfp_lib, world)
    for t in range(FRAMES * 256 // T):
        c.push(T)
        st0 = c.lv.stats()
        got, _ = c.check(t)
        assert c.lv.stats() == st0, t  # tfp_live_stats does not move under the call
    assert eng.index_delta_stats()[1] == 1
    u = db["uuids"]
    fr = [c.lv.frames(ch, 0) for ch in range(NCH)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])])
    batch = eng.search_occurrences_batch(np.concatenate(fr), off, c.args["p"], WINDOW, 1, K, GAP, HITS, scopes=SCOPES)
    for ch, clip, s in ((0, A, 20), (0, B, 99), (1, 5, -30), (1, LO.LATE, 81), (2, 1, 12), (2, 1, 89)):
        e = _entry(got[ch], u[clip], s)
        assert e == _entry(batch[ch], u[clip], s), (ch, clip, s)
        assert e["hits"] >= 40 and max(0, s) <= e["first_frame"] < e["last_frame"] < s + LO.NFRAMES[clip], (ch, clip, s, e)
    e = _entry(got[1], u[LO.LATE], 81)
    assert e["overlap"] == 99 and e["last_frame"] > 81 + 48  # cut by the call's end, not by the clip's
    assert _entry(got[1], u[5], -30)["overlap"] == 71
    st = c.lv.occurrence_stats()
    assert st["calls"] == FRAMES * 256 // T and st["retraces"] == 0
    c.close()


def test_calls_launch_no_fingerprint(tfp_lib, world):
    eng = world[0]
    c = Call(tfp_lib, world)
    c.push(70 * 256 + 100)
    fp0, st0 = eng.fingerprint_stats(), c.lv.stats()
    c.check("first")
    c.check("again")
    assert eng.fingerprint_stats() == fp0 and c.lv.stats() == st0
    c.close()


def test_irregular_ticks(tfp_lib, world):
    """1 sample, 255, 256, 257, then one tick of 64 * 256 + 100 samples (more than 64 frames become final at
    once: the catch-up takes a second step of the kernel's fold), then uneven ticks to the end."""
    c = Call(tfp_lib, world)
    sizes = [1, 255, 256, 257, 40 * 256 - 1, 64 * 256 + 100, 1, 155, 4000, 4097, 513, 9000]
    for n in sizes:
        c.push(n)
        c.check(n)
    c.push(FRAMES * 256 - c.at)
    c.check("end")
    assert c.lv.occurrence_stats()["frames_traced"] > 64
    c.close()


def test_late_first_call_catches_up(tfp_lib, world):
    c = Call(tfp_lib, world)
    for _ in range(15):
        c.push(8 * 256)  # 120 frames ingested, no occurrence call yet
    assert c.lv.occurrence_stats() == dict.fromkeys(LO.OSTAT_KEYS, 0)
    c.ticks(1, 50)
    st = c.lv.occurrence_stats()
    assert st["tracks_added"] >= 3 and st["frames_traced"] >= 40  # every new track from its lo
    c.ticks(30)
    c.close()


def test_tail_that_hits_and_tail_that_does_not(tfp_lib, world):
    """The provisional tail joins the answer, not the stored summary: over ticks of 160 samples, tracks whose
    span holds the tail are seen both with the tail hitting (one hit more than the trace of the final frames
    alone) and with it missing."""
    eng, db, _ = world
    c = Call(tfp_lib, world)
    c.push(60 * 256)
    seen = set()
    for t in range(32):
        c.push(T)
        c.check(t)
        for ch in range(NCH):
            S = c.lv.samples(ch)
            if S % 256 == 0:
                continue
            Ff = S // 256
            fr = c.lv.frames(ch, 0)[:Ff]
            for tr in c.lv.tracks(ch):
                n = db["nrows"][_uuid(eng, db, tr["clip_id"])]
                if not max(0, tr["start"]) <= Ff < tr["start"] + n:
                    continue
                final = eng.trace_batch(fr, [0, Ff], c.args["p"], [(0, tr["clip_id"], tr["start"])], GAP)[0]
                assert tr["hits"] - final["hits"] in (0, 1)
                seen.add(tr["hits"] - final["hits"])
    assert seen == {0, 1}
    c.close()


def _uuid(eng, db, clip_id):
    """The uuid of an engine clip id of the DB (ids follow the order of enrolment, and LATE is the last clip)."""
    return db["uuids"][clip_id]


def test_max_gap_and_tolerance_changes_retrace(tfp_lib, world):
    c = Call(tfp_lib, world)
    c.push(50 * 256)
    c.args["max_gap"] = 0
    c.ticks(8, where="gap 0")
    assert c.lv.occurrence_stats()["retraces"] == 0
    c.args["max_gap"] = INT32_MAX
    got, _ = c.ticks(5, where="gap max")
    assert c.lv.occurrence_stats()["retraces"] == 1
    assert all(tr["segments"] <= 1 for ch in range(NCH) for tr in c.lv.tracks(ch))  # one segment per diagonal
    c.args["p"] = tfp_lib.params(1, 0.001)
    c.ticks(3, where="tolerance")
    c.args["p"] = tfp_lib.params(1, 0.45)
    c.ticks(3, where="tolerance again")
    c.args["p"] = tfp_lib.params(1, 0.45, 3, 0)
    c.ticks(2, where="ignore threshold")
    st = c.lv.occurrence_stats()
    assert st["retraces"] == 4
    # what needs no retrace: k, window, min_hits, max_tracks
    c.args.update(k=1, window=20, min_hits=3, max_tracks=7)
    c.ticks(3, where="k, window, min_hits, max_tracks")
    assert c.lv.occurrence_stats()["retraces"] == 4
    c.close()


def test_max_tracks_bounds_the_list(tfp_lib, world):
    c = Call(tfp_lib, world)
    c.args["max_tracks"] = 2
    dropped = 0
    for t in range(0, FRAMES * 256 // T, 3):
        c.push(3 * T)
        dropped += sum(c.check(t)[1])
    assert dropped > 0 and c.lv.occurrence_stats()["tracks_dropped"] == dropped
    assert all(len(c.lv.tracks(ch)) <= 2 for ch in range(NCH))
    # a lower bound than a list's length drops nothing and only stops additions
    assert max(len(c.lv.tracks(ch)) for ch in range(NCH)) == 2
    c.args["max_tracks"] = 1
    c.check("lowered")
    assert max(len(c.lv.tracks(ch)) for ch in range(NCH)) == 2
    c.close()


def test_reset_of_one_channel(tfp_lib, world):
    c = Call(tfp_lib, world)
    c.push(80 * 256 + 77)
    c.check("before")
    assert all(len(c.lv.tracks(ch)) for ch in range(NCH))
    others = [c.lv.tracks(ch) for ch in (0, 2)]
    c.lv.reset(1)
    c.ref.reset(1)
    c.hist[1] = np.zeros(0, np.int16)
    assert c.lv.tracks(1) == [] and [c.lv.tracks(ch) for ch in (0, 2)] == others
    c.check("after the reset")
    # the channel's new call: clip 5 (of its context) from its start, three times the others' pace
    new = c.db["pcm"][5][:30 * 3 * T]
    for t in range(30):
        blk = np.zeros((NCH, 3 * T), np.int16)
        blk[1] = new[t * 3 * T:(t + 1) * 3 * T]
        blk[0, :T], blk[2, :T] = c.src[0, c.at:c.at + T], c.src[2, c.at:c.at + T]
        c.at += T
        W.push_all(c.lv, c.hist, blk, nsamples=[T, 3 * T, T])
        got, _ = c.check(("new call", t))
    e = _entry(got[1], c.db["uuids"][5], 0)
    assert e["first_frame"] <= 4 and e["last_frame"] >= 48 and e["overlap"] == 30 * 3 * T // 256 + 1, e
    c.close()


def test_index_updates_between_calls(tfp_lib, monkeypatch):
    """A clip enrolled (a copy of the playing clip under the greatest uuid, into the delta), a clip removed (its
    tracks leave) and a tfp_index_commit merge between calls, on an engine of this test's own."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")
    eng = tfp_lib.Engine(0)
    db = LO.build_db(tfp_lib, eng)
    c = Call(tfp_lib, (eng, db, calls(tfp_lib, db)))
    c.push(60 * 256)
    c.ticks(4, where="start")
    u = db["uuids"]
    top = "ffffffff-3333-4000-8000-0000000000ff"
    fr = eng.fingerprint(db["pcm"][A])
    eng.index_add(top, fr["m1"], fr["m2"])
    eng.index_set_scope([top], [0])
    c.ref.enrolled.add(top)
    c.ref.nrows[top] = len(fr)
    c.ref.scope[top] = 0
    got, _ = c.ticks(4, where="enrolment")
    r0 = c.lv.occurrence_stats()["retraces"]
    assert r0 >= 1
    assert _entry(got[0], top, 20) == _entry(got[0], u[A], 20)  # the copy, from the delta's staged rows
    eng.index_remove(u[A])
    c.ref.enrolled.discard(u[A])
    got, _ = c.ticks(4, where="removal")
    assert all(o["audio_uuid"] != u[A] for ch in range(NCH) for o in got[ch])
    assert all(t["clip_id"] != A for ch in range(NCH) for t in c.lv.tracks(ch))
    assert _entry(got[0], top, 20)["hits"] >= 30
    assert c.lv.occurrence_stats()["retraces"] >= r0 + 1
    eng.index_commit()
    c.ticks(4, where="merge")
    c.ticks(30, where="on")
    c.close()
    eng.close()


def test_scope_change_filters_without_retrace(tfp_lib, world):
    c = Call(tfp_lib, world)
    c.push(40 * 256)
    c.ticks(6, size=10 * 256, where="own contexts")  # (every played clip inside a window while it plays)
    got, _ = c.ticks(3, where="own contexts")
    u = c.db["uuids"]
    assert _entry(got[0], u[A], 20) and _entry(got[1], u[5], -30) and _entry(got[2], u[1], 12)
    c.args["scopes"] = [0, 0, 77]  # (channel 1: a context its clips are not in; 77: no clip's scope)
    got, _ = c.ticks(3, where="other scopes")
    for ch, scope in enumerate(c.args["scopes"]):
        assert all(c.db["scope"][o["audio_uuid"]] == scope for o in got[ch]), ch
    assert _entry(got[0], u[A], 20) and got[2] == []
    assert any(t["clip_id"] == 5 and t["start"] == -30 for t in c.lv.tracks(1))  # filtered from the output, kept on the list
    c.args["scopes"] = None  # TFP_SCOPE_ANY
    got, _ = c.ticks(3, where="any")
    assert _entry(got[1], u[5], -30) and _entry(got[2], u[1], 12) and c.lv.occurrence_stats()["retraces"] == 0
    c.close()


def test_coefs_2(tfp_lib, world):
    c = Call(tfp_lib, world)
    c.args["p"] = tfp_lib.params(2, 0.45)
    c.push(40 * 256)
    c.ticks(40, size=2 * T)
    st = c.lv.window_aligned_stats()
    assert st["general_calls"] == 40 and st["inplace_calls"] == 0
    c.close()


def test_alternation_leaves_the_window_calls_unchanged(tfp_lib, world):
    """window, window_aligned and occurrences alternate on one object; a twin fed the same pushes answers only
    the window calls: their outputs are equal, and so are both window counters but for the calls counted."""
    eng = world[0]
    c = Call(tfp_lib, world)
    twin = tfp_lib.Live(eng, NCH, FRAMES * 256)
    p = c.args["p"]
    for t in range(60):
        blk = c.src[:, c.at:c.at + 2 * T]
        assert twin.push(blk, None) is None
        c.push(2 * T)
        if t % 3 == 0:
            c.check(t)
        w = 7 if t % 4 == 0 else WINDOW
        assert c.lv.window(p, None, K, w) == twin.window(p, None, K, w), t
        if t % 2:
            c.check(t)
        assert c.lv.window_aligned(p, None, K, w) == twin.window_aligned(p, None, K, w), t
    a, b = c.lv.window_stats(), twin.window_stats()
    assert a["general_calls"] == b["general_calls"] == 0 and a["slid_calls"] == b["slid_calls"] + c.lv.occurrence_stats()["calls"]
    twin.close()
    c.close()


def test_steady_state_cost_is_the_tracks_in_span(tfp_lib, world):
    """20 single-frame ticks with no new track (max_tracks below every list's length stops additions):
    frames_traced grows by exactly the tracks whose span holds the newly final frame, whatever the call's age."""
    eng, db, _ = world
    c = Call(tfp_lib, world)
    c.push(100 * 256)
    c.check("populate")
    assert all(len(c.lv.tracks(ch)) >= 2 for ch in range(NCH))
    c.args["max_tracks"] = 1
    grown = 0
    for t in range(20):
        before = c.lv.occurrence_stats()
        c.push(256)
        c.check(t)
        after = c.lv.occurrence_stats()
        assert after["tracks_added"] == before["tracks_added"]
        x = c.at // 256 - 1  # the frame that became final
        exp = sum(1 for ch in range(NCH) for tr in c.lv.tracks(ch)
                  if max(0, tr["start"]) <= x < tr["start"] + db["nrows"][_uuid(eng, db, tr["clip_id"])])
        assert after["frames_traced"] - before["frames_traced"] == exp, (t, x)
        grown += exp
    assert 0 < grown <= 20 * sum(len(c.lv.tracks(ch)) for ch in range(NCH))
    c.close()


def test_argument_errors_move_nothing(tfp_lib, world):
    eng = world[0]
    c = Call(tfp_lib, world)
    c.push(70 * 256 + 9)
    c.check("before")
    lib = tfp_lib.lib()
    p = tfp_lib.params(1, 0.45)
    h = c.lv._h
    st = (c.lv.occurrence_stats(), c.lv.window_stats(), c.lv.window_aligned_stats(), [c.lv.tracks(ch) for ch in range(NCH)])
    out = (tfp_lib.engine.Occurrence * 8)()
    out[0].hits = 123
    n, drop = C.c_int64(-7), (C.c_int32 * NCH)(5, 5, 5)
    ok = dict(p=C.byref(p), sc=None, k=K, w=WINDOW, g=GAP, m=HITS, mt=64, out=out, cap=8, n=C.byref(n), d=drop)
    bad_scopes = (C.c_int32 * NCH)(-1, -2, 0)
    for change in (dict(k=0), dict(k=33), dict(w=0), dict(g=-1), dict(m=0), dict(mt=0), dict(mt=65), dict(sc=bad_scopes),
                   dict(p=None), dict(out=None), dict(n=None)):
        a = dict(ok, **change)
        rc = lib.tfp_live_occurrences(h, a["p"], a["sc"], a["k"], a["w"], a["g"], a["m"], a["mt"], a["out"], a["cap"], a["n"], a["d"])
        assert rc == -1, change
        assert n.value == -7 and list(drop) == [5, 5, 5] and out[0].hits == 123, change
        assert st == (c.lv.occurrence_stats(), c.lv.window_stats(), c.lv.window_aligned_stats(),
                      [c.lv.tracks(ch) for ch in range(NCH)]), change
    assert "live occurrences" in eng.last_error()
    # invalid params: no rows, nothing offered, the lists stay
    got, dropped = c.lv.occurrences(tfp_lib.params(3, 0.45), None, K, WINDOW, GAP, HITS, 64)
    assert got == [[], [], []] and dropped == [0, 0, 0] and st[3] == [c.lv.tracks(ch) for ch in range(NCH)]
    c.ref.exp["calls"] += 1
    # a capacity below the list: TFP_E_CAPACITY names the room it needs
    with pytest.raises(tfp_lib.TfpError) as ei:
        c.lv.occurrences(p, None, K, WINDOW, GAP, HITS, 64, cap=0)
    assert ei.value.code == -5
    c.close()


def test_empty_index_and_idle_channel(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng = tfp_lib.Engine(0)
    lv = tfp_lib.Live(eng, 2, 9000)
    clip = LO.clip_pcm(tfp_lib, 0)[:4000]
    blk = np.stack([clip, clip])
    assert lv.push(blk, None, nsamples=[4000, 0]) is None
    p = tfp_lib.params(1, 0.45)
    assert lv.occurrences(p, None, K, WINDOW, GAP, HITS, 64) == ([[], []], [0, 0])
    assert lv.tracks(0) == [] and lv.tracks(1) == []
    fr = eng.fingerprint(clip)
    assert len(fr) == 16
    eng.index_add("00000000-3333-4000-8000-000000000001", fr["m1"], fr["m2"])
    got, _ = lv.occurrences(p, None, K, WINDOW, GAP, 1, 64)
    tr = lv.tracks(0)
    assert len(tr) == 1 and len(got[0]) == 1 and got[1] == [] and lv.tracks(1) == []
    s = tr[0]["start"]
    # the final frames [0, 15) inside the span, the tail (frame 15) joined on top and not counted
    assert lv.occurrence_stats()["frames_traced"] == max(0, min(15, s + 16) - max(0, s))
    lv.close()
    eng.close()
