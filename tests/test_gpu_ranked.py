"""Ranked search (tfp_search_ranked*, csrc/tfp_rank.hip): the first k rows of the reference's result
query "select *, count(*) from temp group by audio_uuid order by count(*) DESC" (fp_handler.c:367-374)
against the SQLite-peeled fixture tests/golden/ranked_cases.json and a brute-force count."""
import ctypes as C

import numpy as np
import pytest

import ranked_util as R

pytestmark = pytest.mark.gpu

TFP_E_ARG = -1


def _raw(tfp_lib, eng, frames, p, k):
    """tfp_search_ranked as the C caller sees it: (rc, out[k], count)."""
    from tiresias_amd._lib import Candidate
    frames = np.ascontiguousarray(frames, R.FRAME_DTYPE)
    out, count = (Candidate * k)(), C.c_int32(-7)
    C.memset(out, 0xFF, C.sizeof(out))  # the call must zero what it does not fill
    rc = tfp_lib.lib().tfp_search_ranked(eng.handle, frames.ctypes.data, len(frames), C.byref(p), k, out, C.byref(count))
    return rc, out, count.value


def _rows(out, n):
    return [(c.uuid.decode(), c.match_count) for c in out[:n]]


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def test_goldens_every_query_k_1_3_8(engine, tfp_lib):
    scen, ranked = R.load_cases()
    n = 0
    for name, s in scen.items():
        R.enrol(engine, s)
        for qi, q in enumerate(s["queries"]):
            exp = ranked[(name, qi)]
            fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
            plain, fc = engine.search(fr, p)
            assert fc == q["frame_count"]
            if q["coefs"] not in (1, 2):
                assert _raw(tfp_lib, engine, fr, p, 3)[0] == TFP_E_ARG and plain is None and exp == []
                continue
            for k in (1, 3, 8):
                rc, out, cnt = _raw(tfp_lib, engine, fr, p, k)
                assert rc == 0, (name, qi, k, engine.last_error())
                assert cnt == min(k, len(exp)) and _rows(out, cnt) == exp[:k], (name, qi, k)
                assert bytes(out)[cnt * C.sizeof(out[0]):] == bytes((k - cnt) * C.sizeof(out[0])), (name, qi, k)
                row0 = None if plain is None else (plain["audio_uuid"], plain["match_count"], plain["clip_id"])
                got0 = (out[0].uuid.decode(), out[0].match_count, out[0].clip_id) if cnt else None
                assert got0 == row0, (name, qi, k)
            n += 1
    engine.index_clear()
    assert n > 850


def _one_row_index(engine, C_):
    """C_ one-row clips, column c = clip c (uuids ascending), clip c's row in key 10 + c % 5."""
    uuids = ["00000000-0000-4000-8000-%012d" % c for c in range(C_)]
    m1 = np.array([(10 + c % 5) * 1_000_000 + 500 for c in range(C_)], np.int32)
    m2 = np.zeros(C_, np.int32)
    engine.index_clear()
    engine.index_add_batch(uuids, np.arange(C_ + 1), m1, m2)
    return uuids, m1, m2


def test_block_and_merge_boundaries(engine, tfp_lib, oracle):
    scen, ranked = R.load_cases()
    s = scen["tie_2000"]  # 2,000 columns: two column chunks
    R.enrol(engine, s)
    top = sorted(s["uuids"], reverse=True)[:8]
    for qi, q in enumerate(s["queries"]):
        got = R.pairs(engine.search_ranked(R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q), 8))
        assert got == ranked[("tie_2000", qi)], qi
        if got:
            assert [u for u, _ in got] == top and len({n for _, n in got}) == 1, qi
    assert ranked[("tie_2000", 0)]
    # key 10 + j in j + 1 frames: clip c counts c % 5 + 1, so the top rows are the clips with c % 5 == 4
    # from the greatest uuid down: at C = 1025 column 1024 (the second chunk's only column) leads
    # columns of the first chunk
    q1 = [10.2 + j for j in range(5) for _ in range(j + 1)]
    q2 = [0.0] * len(q1)
    p = tfp_lib.params(1, 0.001)
    for C_ in (1023, 1024, 1025):
        uuids, m1, m2 = _one_row_index(engine, C_)
        exp = R.brute_force(oracle, uuids, np.arange(C_), m1, m2, q1, q2, 1, 0.001, -1, -1)
        assert len(exp) == C_
        for k in (1, 8, 32):
            got = R.pairs(engine.search_ranked(R.frames_from_q(q1, q2), p, k))
            assert got == exp[:k], (C_, k)
        if C_ == 1025:
            assert exp[0][0] == uuids[1024] and exp[1][0] == uuids[1019]
    engine.index_clear()


def test_form_selection_and_scratch_restored(tfp_lib, oracle, monkeypatch):
    monkeypatch.setenv("TFP_WIDE_MIN_TOL", "1e9")  # plain general-path searches take the cells form / row scan
    scen, ranked = R.load_cases()
    name = "rand_05"
    s = scen[name]
    with tfp_lib.Engine(0) as eng:
        R.enrol(eng, s)
        by_coefs = {c: [qi for qi, q in enumerate(s["queries"]) if q["coefs"] == c and ranked[(name, qi)]] for c in (1, 2)}
        assert by_coefs[1] and by_coefs[2]
        qi = next(i for i in by_coefs[1] if s["queries"][i]["tol"] == 0.001)
        q = s["queries"][qi]
        st0 = eng.rank_stats()
        assert R.pairs(eng.search_ranked(R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q), 8)) == ranked[(name, qi)]
        st1 = eng.rank_stats()
        assert (st1["vote_batches"], st1["general_batches"]) == (st0["vote_batches"] + 1, st0["general_batches"])
        for qi in by_coefs[2]:
            q = s["queries"][qi]
            assert R.pairs(eng.search_ranked(R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q), 8)) == ranked[(name, qi)]
        st2 = eng.rank_stats()
        assert (st2["vote_batches"], st2["general_batches"]) == (st1["vote_batches"], st1["general_batches"] + len(by_coefs[2]))
        # the scan scratch is zero again: plain coefs = 2 searches on the same engine match the goldens
        for qi, q in enumerate(s["queries"]):
            if q["coefs"] == 2:
                r, _ = eng.search(R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q))
                got = None if r is None else {"audio_uuid": r["audio_uuid"], "match_count": r["match_count"],
                                              "frame_count": r["frame_count"]}
                assert got == q["expect"], qi
        # a 600.0 dB query frame: a key outside the vote range, served by the general form
        uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(3)]
        m1 = [600_000_100, 24_000_000, 600_000_200, 24_000_100, 24_000_200]
        clip = [0, 0, 1, 2, 2]
        eng.index_clear()
        for c in range(3):
            eng.index_add(uuids[c], np.array([m for m, k in zip(m1, clip) if k == c], np.int32),
                          np.zeros(clip.count(c), np.int32))
        q1, q2 = [600.0, 24.5, 24.7], [0.0, 0.0, 0.0]
        exp = R.brute_force(oracle, uuids, clip, m1, [0] * 5, q1, q2, 1, 0.001, -1, -1)
        assert exp == [(uuids[0], 3), (uuids[2], 2), (uuids[1], 1)]
        st3 = eng.rank_stats()
        assert R.pairs(eng.search_ranked(R.frames_from_q(q1, q2), tfp_lib.params(1, 0.001), 8)) == exp
        st4 = eng.rank_stats()
        assert (st4["vote_batches"], st4["general_batches"]) == (st3["vote_batches"], st3["general_batches"] + 1)


def test_index_delta(tfp_lib, monkeypatch):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    scen, ranked = R.load_cases()
    name = max((n for n in scen if n.startswith("rand_")), key=lambda n: len(scen[n]["uuids"]))
    s = scen[name]
    nc = len(s["uuids"])
    assert nc >= 10
    clip = np.asarray(s["clip"], np.int64)
    m1 = np.asarray(s["m1"], np.int64).astype(np.int32)
    m2 = np.asarray(s["m2"], np.int64).astype(np.int32)
    with tfp_lib.Engine(0) as eng, tfp_lib.Engine(0) as fresh:
        R.enrol(fresh, s)
        for c in range(nc - 3):
            eng.index_add(s["uuids"][c], m1[clip == c], m2[clip == c])
        eng.index_commit()
        eng.search(R.frames_from_q([24.3], [1.0]), tfp_lib.params(1, 0.001))
        for c in range(nc - 3, nc):
            eng.index_add(s["uuids"][c], m1[clip == c], m2[clip == c])
        eng.index_commit()
        assert eng.index_delta_stats()[1] == 3
        n = {1: 0, 2: 0}
        for coefs in (1, 2):  # (coefs = 2 merges the delta: after the coefs = 1 queries)
            for qi, q in enumerate(s["queries"]):
                if q["coefs"] != coefs or q["tol"] != q["tol"] or q["tol"] > 8:
                    continue
                fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
                got = R.pairs(eng.search_ranked(fr, p, 8))
                assert got == R.pairs(fresh.search_ranked(fr, p, 8)) == ranked[(name, qi)], (coefs, qi)
                n[coefs] += bool(got)
            if coefs == 1:
                assert eng.index_delta_stats()[1] == 3  # served beside the index, not merged
        assert n[1] > 3 and n[2] > 0


def test_peel_on_the_device(engine, tfp_lib):
    scen, ranked = R.load_cases()
    name = "rand_05"
    s = scen[name]
    qi = max(range(len(s["queries"])), key=lambda i: len(ranked[(name, i)]))
    q = s["queries"][qi]
    assert len(ranked[(name, qi)]) >= 3
    R.enrol(engine, s)
    fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
    before = R.pairs(engine.search_ranked(fr, p, 32))
    assert before[:8] == ranked[(name, qi)]
    engine.index_remove(before[0][0])
    assert R.pairs(engine.search_ranked(fr, p, 32)) == before[1:]
    engine.index_clear()


def test_arguments(engine, tfp_lib, oracle):
    _one_row_index(engine, 40)
    q1 = [10.2 + j for j in range(4) for _ in range(j + 1)]  # key 14's 8 clips score nothing
    fr = R.frames_from_q(q1, [0.0] * len(q1))
    for k, coefs in ((0, 1), (33, 1), (-1, 1), (4, 3), (4, 0)):
        from tiresias_amd._lib import Candidate
        out, cnt = (Candidate * 40)(), C.c_int32()
        p = tfp_lib.params(coefs, 0.001)
        rc = tfp_lib.lib().tfp_search_ranked(engine.handle, fr.ctypes.data, len(fr), C.byref(p), k, out, C.byref(cnt))
        assert rc == TFP_E_ARG, (k, coefs)
    got = engine.search_ranked(fr, tfp_lib.params(1, 0.001), 32)
    assert len(got) == 32  # k = TFP_RANK_MAX on 40 clips
    fewer = engine.search_ranked(R.frames_from_q([10.2], [0.0]), tfp_lib.params(1, 0.001), 32)
    assert len(fewer) == 8 and all(r["match_count"] == 1 for r in fewer)  # every scoring clip
    engine.index_clear()


def test_batch_equals_single_calls(engine, tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    R.enrol(engine, s)
    qs = [q for q in s["queries"] if q["coefs"] == 1][:8]
    lens = sorted({len(q["q1"]) for q in qs})
    assert len(lens) > 4
    frames = [R.frames_from_q(q["q1"], q["q2"]) for q in qs]
    frames.insert(4, R.frames_from_q([], []))  # nine queries, one of them empty
    qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        batch = engine.search_ranked_batch(np.concatenate(frames), qoff, p, 5)
        assert len(batch) == 9 and batch[4] == [] and any(len(b) > 1 for b in batch)
        for i, f in enumerate(frames):
            assert batch[i] == engine.search_ranked(f, p, 5), i
    engine.index_clear()


def test_group_of_three_equals_fixture(tfp_lib):
    scen, ranked = R.load_cases()
    g = tfp_lib.Group([0, 0, 0])
    try:
        n = 0
        for name, s in scen.items():
            R.enrol(g, s)
            by_p = {}
            for qi, q in enumerate(s["queries"]):
                if q["coefs"] in (1, 2):
                    by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
            for qis in by_p.values():  # the queries of one parameter set as one batch
                q0 = s["queries"][qis[0]]
                frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis]
                qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
                got = g.search_ranked_batch(np.concatenate(frames), qoff, _params(tfp_lib, q0), 8)
                for i, rows in zip(qis, got):
                    assert R.pairs(rows) == ranked[(name, i)], (name, i)
                    n += 1
            if name == "tie_2000":
                assert len({r["clip_id"] for rows in got for r in rows}) > 1  # the tied rows come from several shards
        assert n > 850
    finally:
        g.close()


def test_pcm_form_equals_frames_form(engine, tfp_lib, oracle):
    n = 8000 * 5
    seen = 0
    pcm = tfp_lib.synth_pcm(0x7153A1, range(2), n)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(3) * n)
    nf = len(fr) // 2
    uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(2)]
    engine.index_clear()
    for c in range(2):
        engine.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    q = np.ascontiguousarray(pcm[:, :16000]).reshape(-1)
    off = np.arange(3) * 16000
    qfr = engine.fingerprint_batch(q, off)
    qoff = np.arange(3) * (len(qfr) // 2)
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        got = engine.search_ranked_pcm_batch(q, off, p, 2)
        assert got == engine.search_ranked_batch(qfr, qoff, p, 2)
        for i in range(2):  # (a clip's first 2 s need not match it: the box is around the truncated value)
            f = qfr[qoff[i]:qoff[i + 1]]
            exp = R.brute_force(oracle, uuids, np.repeat([0, 1], nf), fr["m1"], fr["m2"], list(f["q1"]), list(f["q2"]),
                                p.coefs, 0.45, -1, -1, limit=2)
            assert R.pairs(got[i]) == exp, (p.coefs, i)
            seen += len(exp)
    assert seen > 0
    engine.index_clear()
