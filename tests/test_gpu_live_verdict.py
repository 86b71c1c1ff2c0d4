"""The early verdict of a live call (tfp_live_verdict, live_verdict_kernel in csrc/tfp_live.hip): after
every push each channel's verdict equals the rule of tiresias_fp.h restated in verdict_util over the
CPU oracle's brute-force counts of the call's final frames, field for field, and a decided verdict
names the first row of tfp_search_scoped_pcm_batch on the finished recording
(application_handler.c:163, :248-312; fp_handler.c:287-374 with the context predicate at :308-314)."""
import numpy as np
import pytest

import live_util as L
import verdict_util as V

pytestmark = pytest.mark.gpu

TFP_E_ARG = -1
T = V.T


@pytest.fixture(scope="module")
def data(oracle):
    runs = V.assert_data(oracle)  # the conditions on the input, on the CPU oracle alone, before any GPU call
    return V.db(oracle), runs


@pytest.fixture(scope="module")
def eng(tfp_lib, data):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    e = tfp_lib.Engine(0)
    V.enrol(e, data[0])
    yield e
    e.close()


def _tick(pcms, at, n):
    """One push's block: channel c's next n[c] samples, the rest of the row never read."""
    blk = np.full((len(pcms), max(max(n), 1)), 12345, np.int16)
    for c, x in enumerate(pcms):
        blk[c, :n[c]] = x[at[c]:at[c] + n[c]]
    return blk


def test_every_push_equals_the_oracle_and_decided_is_final(eng, tfp_lib, oracle, data):
    """8 channels of differing totals (total % 256 in {0, 1, 255}, a single tick, total == max_samples):
    every push's verdict equals the oracle's; from the first decided push on the leader stays, and it is
    the first row of the scoped search of the whole recording."""
    d, runs = data
    p = tfp_lib.params(1, V.TOL)
    totals = [c[2] for c in V.CALLS]
    scopes = [c[1] for c in V.CALLS]
    assert {t % 256 for t in totals} >= {0, 1, 255} and 160 in totals and V.MAX_SAMPLES in totals
    pcms = [V.call_pcm(i) for i in range(8)]
    lv = tfp_lib.Live(eng, 8, V.MAX_SAMPLES)
    at = [0] * 8
    first_decided = [None] * 8
    seen_early = False
    for t in range(max(len(r) for r in runs)):
        n = [min(T, totals[c] - at[c]) for c in range(8)]
        lv.push(_tick(pcms, at, n), None, nsamples=n)
        at = [at[c] + n[c] for c in range(8)]
        got = lv.verdict(totals, p, scopes)
        for c in range(8):
            exp = runs[c][min(t, len(runs[c]) - 1)]
            assert V.as_oracle(got[c]) == exp, (t, c, at[c])
            if got[c]["decided"] and got[c]["leader"]:
                first_decided[c] = first_decided[c] or got[c]["leader"]["audio_uuid"]
                assert got[c]["leader"]["audio_uuid"] == first_decided[c], (t, c)
                seen_early |= not got[c]["complete"]
    assert seen_early
    off = np.concatenate([[0], np.cumsum(totals)])
    rows = eng.search_scoped_pcm_batch(np.concatenate(pcms), off, p, scopes, 1)
    for c in range(8):
        assert at[c] == totals[c]
        if first_decided[c]:
            assert rows[c][0]["audio_uuid"] == first_decided[c], c
        else:
            assert rows[c] == [], c
    # the switch call: undecided for as long as its first clip's best match leads
    sw = runs[4]
    a = sw[5]["leader"][0]
    assert a != sw[-1]["leader"][0] and not any(v["decided"] for v in sw if v["leader"] and v["leader"][0] == a)
    # the scope of a single clip: no rival, decided from the first hit
    lone = runs[6]
    hit = next(i for i, v in enumerate(lone) if v["leader"])
    assert all(v["rival"] is None and v["decided"] for v in lone[hit:]) and not lone[hit]["complete"]
    st = lv.stats()
    assert st["rebuilds"] == 1 and st["general_pushes"] == 0 and st["frames_added"] == sum(t // 256 for t in totals)
    lv.close()


def test_twins_removed_clip_and_rowless_clip(eng, tfp_lib, oracle, data):
    """The twins tie at every push with the greater uuid leading; under TFP_SCOPE_ANY the removed clip
    (the greatest uuid of all before its removal, playing in the call) and the row-less clip are no
    candidates."""
    d, runs = data
    tw = runs[2]
    assert any(v["leader"] and v["rival"] and {v["leader"][0], v["rival"][0]} == {V.uuid_of(c) for c in V.TWIN} and
               v["leader"][1] == v["rival"][1] and v["leader"][0] > v["rival"][0] for v in tw)
    for v in runs[3]:  # the call that plays the removed clip, over every scope
        for side in ("leader", "rival"):
            assert v[side] is None or v[side][0] not in (V.uuid_of(V.REMOVED), V.uuid_of(V.ROWLESS))
    # a scope holding only the row-less clip and the removed clip's scope mates: the row-less clip never shows,
    # not even as a rival with count 0 (its uuid is above several of scope 2's candidates)
    p = tfp_lib.params(1, V.TOL)
    x = V.clip_pcm(20)[:1600]
    lv = tfp_lib.Live(eng, 1, 4096)
    for i in range(10):
        lv.push(x[None, i * T:(i + 1) * T], None)
        got = V.as_oracle(lv.verdict([4096], p, [2])[0])
        assert got == V.verdict(oracle, d, x[:(i + 1) * T], 4096, V.TOL, 2, V.ALIVE), i
    lv.close()


def test_zero_count_rival_decides(eng, tfp_lib, oracle, data):
    """Scope ZSCOPE holds the clip the call plays and a clip of another kind with the greater uuid, whose
    count stays 0: while leader.count == remaining the rival's tie key keeps the call undecided, one
    frame later it is decided. A kernel that drops score-0 columns sees no rival and decides at once."""
    d, _ = data
    p = tfp_lib.params(1, V.TOL)
    total = 4096
    x = V.clip_pcm(V.ZLEAD)[:total]
    lv = tfp_lib.Live(eng, 2, total)
    edge = None
    for i, S in enumerate(V.lengths(total)):
        n = S - i * T
        lv.push(np.stack([x[i * T:i * T + n], x[i * T:i * T + n]]), None)
        got = [V.as_oracle(v) for v in lv.verdict([total, total], p, [V.ZSCOPE, V.ZSCOPE])]
        exp = V.verdict(oracle, d, x[:S], total, V.TOL, V.ZSCOPE, V.ALIVE)
        assert got == [exp, exp], S
        if exp["leader"] and exp["leader"][1] == exp["remaining"]:
            assert exp["rival"] == (V.uuid_of(V.ZRIVAL), 0) and not exp["decided"]
            edge = S // 256
        elif edge is not None and S // 256 == edge + 1:
            assert exp["decided"] and not exp["complete"]
    assert edge is not None
    lv.close()


def test_empty_index_and_argument_errors(tfp_lib, oracle, data):
    d, _ = data
    eng = tfp_lib.Engine(0)
    p = tfp_lib.params(1, V.TOL)
    lv = tfp_lib.Live(eng, 2, 1024)
    x = V.clip_pcm(6)[:1024]
    lv.push(np.stack([x[:300], x[:300]]), None, nsamples=[300, 200])
    got = lv.verdict([1024, 200], p)  # the empty index: no leader anywhere, decided = complete
    assert [(v["leader"], v["rival"], v["remaining"], v["complete"], v["decided"]) for v in got] == \
        [(None, None, 3, False, False), (None, None, 0, True, True)]
    V.enrol(eng, d)
    for tot, pp, sc in (([299, 1024], p, None), ([1024, 1025], p, None), ([1024, 1024], tfp_lib.params(2, V.TOL), None),
                        ([1024, 1024], tfp_lib.params(3, V.TOL), None), ([1024, 1024], p, [0, -2]), ([1024, 1024], None, None)):
        rc, raw = V.raw_verdict(tfp_lib, lv, tot, pp, sc)
        assert rc == TFP_E_ARG, (tot, sc)
        assert all(v.remaining == 77 and v.decided == 77 and v.has_leader == 77 for v in raw)
    with pytest.raises(tfp_lib.TfpError) as ei:
        lv.verdict([299, 1024], p)
    assert ei.value.code == TFP_E_ARG
    assert lv.stats()["rebuilds"] == 0  # a refused verdict brings nothing up to date
    assert V.as_oracle(lv.verdict([1024, 1024], p, [0, 0])[0]) == V.verdict(oracle, d, x[:300], 1024, V.TOL, 0, V.ALIVE)
    lv.close()
    eng.close()


def test_scope_any_over_columns_without_a_clip(tfp_lib, oracle, data, monkeypatch):
    """One clip with rows in the main index, then the row-less clip and (enrolled, then removed) the
    greatest uuid in the index delta: under TFP_SCOPE_ANY the delta's unused columns, the row-less
    clip's and the removed clip's are no candidates, so there is no rival and the first hit decides.
    A kernel that admits columns without a candidate reports a rival of count 0 here."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")
    d, _ = data
    eng = tfp_lib.Engine(0)
    V.enrol(eng, d, only=[V.LONE])
    eng.index_commit()
    for c in (V.ROWLESS, V.REMOVED):
        sel = d["clip"] == c
        eng.index_add(V.uuid_of(c), d["m1"][sel].astype(np.int32), d["m2"][sel].astype(np.int32))
    eng.index_remove(V.uuid_of(V.REMOVED))
    p = tfp_lib.params(1, V.TOL)
    x = V.clip_pcm(V.LONE)[768:768 + 2560]
    lv = tfp_lib.Live(eng, 1, 2560)
    hits = 0
    for i in range(16):
        lv.push(x[None, i * T:(i + 1) * T], None)
        got = V.as_oracle(lv.verdict([2560], p, [-1])[0])
        assert got == V.verdict(oracle, d, x[:(i + 1) * T], 2560, V.TOL, -1, [V.LONE, V.ROWLESS]), i
        if got["leader"]:
            hits += 1
            assert got["rival"] is None and got["decided"]
    assert hits and eng.index_delta_stats()[1] >= 1  # the delta holds the row-less clip
    lv.close()
    eng.close()


def test_mid_call_changes_and_pushes_unchanged(tfp_lib, oracle, data, monkeypatch):
    """An enrolment (into the index delta, whose unused columns hold no clip), a removal, a tolerance
    change and a scope change between pushes: the verdict follows each (the count rows are rebuilt exactly
    where a push would rebuild them), and a verdict between two pushes changes nothing the next push shows."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the index delta at this DB size too
    d, _ = data
    eng = tfp_lib.Engine(0)
    V.enrol(eng, d, removed=False, only=[c for c in range(V.NCLIPS) if c != V.REMOVED])
    total = 6400
    x = [V.clip_pcm(V.REMOVED)[256:256 + total], V.clip_pcm(7)[:total]]
    lv = tfp_lib.Live(eng, 2, total)
    hist = [np.zeros(0, np.int16) for _ in range(2)]
    state = {"t": 0, "p": tfp_lib.params(1, V.TOL), "tol": V.TOL, "scopes": [-1, 1], "alive": list(V.ALIVE), "rebuilds": 0}

    def ticks(n, rebuilt, why):
        for _ in range(n):
            t = state["t"]
            blk = np.stack([x[0][t * T:(t + 1) * T], x[1][t * T:(t + 1) * T]])
            if t % 2:  # a searching push: its rows equal the prefix search, verdicts before it or not
                L.check_push(tfp_lib, eng, lv, hist, blk, state["p"], state["scopes"], 3, where=(why, t))
            else:
                lv.push(blk, None)
                for c in range(2):
                    hist[c] = np.concatenate([hist[c], blk[c]])
            got = lv.verdict([total, total], state["p"], state["scopes"])
            for c in range(2):
                exp = V.verdict(oracle, d, hist[c], total, state["tol"], state["scopes"][c], state["alive"])
                assert V.as_oracle(got[c]) == exp, (why, t, c)
            state["t"] += 1
        state["rebuilds"] += rebuilt
        assert lv.stats()["rebuilds"] == state["rebuilds"], why
        return got

    ticks(6, 1, "start")
    # the clip channel 0 plays, the greatest uuid of all, enrolled mid-call: it lands in the delta and leads
    sel = d["clip"] == V.REMOVED
    eng.index_add(V.uuid_of(V.REMOVED), d["m1"][sel].astype(np.int32), d["m2"][sel].astype(np.int32))
    eng.index_set_scope([V.uuid_of(V.REMOVED)], [2])
    state["alive"] = list(range(V.NCLIPS))
    got = ticks(4, 1, "delta enrolment")
    assert eng.index_delta_stats()[1] == 1 and got[0]["leader"]["audio_uuid"] == V.uuid_of(V.REMOVED)
    # ... and removed again: the delta's columns hold no clip now, and it is no candidate
    eng.index_remove(V.uuid_of(V.REMOVED))
    state["alive"] = list(V.ALIVE)
    got = ticks(4, 1, "removal")
    assert got[0]["leader"]["audio_uuid"] != V.uuid_of(V.REMOVED)
    state["p"], state["tol"] = tfp_lib.params(1, 0.3), 0.3
    ticks(4, 1, "tolerance")
    state["scopes"] = [0, 2]
    ticks(4, 0, "scopes")
    eng.index_set_scope([V.uuid_of(7)], [2])
    d2 = dict(d, scope=[2 if c == 7 else s for c, s in enumerate(d["scope"])])
    got = lv.verdict([total, total], state["p"], state["scopes"])
    assert V.as_oracle(got[1]) == V.verdict(oracle, d2, hist[1], total, 0.3, 2, state["alive"])
    assert lv.stats()["rebuilds"] == state["rebuilds"] and lv.stats()["general_pushes"] == 0
    lv.close()
    eng.close()
