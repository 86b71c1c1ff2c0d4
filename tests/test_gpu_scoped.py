"""Context-scoped search (tfp_search_scoped*, csrc/tfp_scope.hip): per query the first k rows of the
reference's result query (fp_handler.c:367-374) over the clips of one scope, i.e. with "and context =
'<s>'" in the per-frame insert (fp_handler.c:308-314), against the SQLite-peeled per-context fixture
tests/golden/scoped_cases.json and a brute-force count over the scope's clips."""
import ctypes as C

import numpy as np
import pytest

import ranked_util as R
import scoped_util as S

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_NOENT = -1, -4
ANY = -1


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _batch(frames):
    return np.concatenate(frames), np.concatenate([[0], np.cumsum([len(f) for f in frames])])


def _scoped(eng, frames, p, scopes, k):
    """One scoped batch: query i = frames[i] in scope scopes[i]; rows as (uuid, count) pairs."""
    fr, qoff = _batch(frames)
    return [R.pairs(rows) for rows in eng.search_scoped_batch(fr, qoff, p, scopes, k)]


def _by_params(s):
    by_p = {}
    for qi, q in enumerate(s["queries"]):
        if q["coefs"] in (1, 2):
            by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
    return by_p


def test_goldens_every_query_each_context_k_1_3_8(engine, tfp_lib, oracle):
    scen, _ = R.load_cases()
    scoped = S.load_scoped()
    n = 0
    for name, s in scen.items():
        S.enrol_scoped(engine, s)
        for qis in _by_params(s).values():  # the queries of one parameter set, each in the three scopes, as one batch
            p = _params(tfp_lib, s["queries"][qis[0]])
            frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in range(S.CONTEXTS)]
            scopes = [x for _ in qis for x in range(S.CONTEXTS)]
            for k in (1, 3, 8):
                got = _scoped(engine, frames, p, scopes, k)
                for j, i in enumerate(qis):
                    for x in range(S.CONTEXTS):
                        assert got[j * S.CONTEXTS + x] == scoped[(name, i)][x][:k], (name, i, x, k)
                        n += 1
        if name == "tie_2000":  # 2,000 clips tied: k = 32 reaches past a context's first rows
            for qi, q in enumerate(s["queries"]):
                fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
                for x in range(S.CONTEXTS):
                    exp = R.brute_force(oracle, *S.restrict(s, x), q["q1"], q["q2"], q["coefs"], q["tol"], q["low"],
                                        q["high"], limit=32)
                    assert exp[:8] == scoped[(name, qi)][x]
                    assert _scoped(engine, [fr], p, [x], 32)[0] == exp, (qi, x)
            assert len(scoped[(name, 0)][0]) == 8
    engine.index_clear()
    assert n > 3 * 3 * 850


def test_scope_any_equals_ranked_and_mixed_batch_equals_single_scope_calls(engine, tfp_lib):
    scen, ranked = R.load_cases()
    scoped = S.load_scoped()
    for name in ("rand_05", "tie_2000"):
        s = scen[name]
        S.enrol_scoped(engine, s)
        for qis in _by_params(s).values():
            p = _params(tfp_lib, s["queries"][qis[0]])
            frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis]
            fr, qoff = _batch(frames)
            plain = engine.search_ranked_batch(fr, qoff, p, 8)
            assert engine.search_scoped_batch(fr, qoff, p, [ANY] * len(qis), 8) == plain  # uuid, count and clip id
            assert [R.pairs(r) for r in plain] == [ranked[(name, i)] for i in qis]
            # one batch mixing the three scopes, ANY and a scope no clip has
            kinds = [0, 1, 2, ANY, S.UNUSED_SCOPE]
            mixed = _scoped(engine, [f for f in frames for _ in kinds], p, kinds * len(qis), 8)
            for x in kinds:
                alone = _scoped(engine, frames, p, [x] * len(qis), 8)
                assert alone == mixed[kinds.index(x)::len(kinds)], (name, x)
                if x == S.UNUSED_SCOPE:
                    assert alone == [[] for _ in qis]
                elif x != ANY:
                    assert alone == [scoped[(name, i)][x] for i in qis]
    engine.index_clear()


def test_scopes_alternate_around_the_chunk_boundary(engine, tfp_lib, oracle):
    """1,030 clips (columns) of 2 or 3 rows, scope c % 2: columns 1023 / 1024 / 1025 alternate across
    the first chunk's end; 1,030 is no multiple of 4 or 32. Every clip scores 2 (ties inside each
    scope); a third row makes a few clips score 3, placed so that each scope's best lies in the first
    chunk for one query and in the second for the other, with the global winner in the other scope."""
    C_ = 1030
    uuids = ["00000000-0000-4000-8000-%012d" % c for c in range(C_)]
    third = {1023: 12, 1026: 12, 4: 13, 1025: 13, 1029: 13}  # column -> key of its third row
    m1, clip = [], []
    for c in range(C_):
        keys = [10, 11] + ([third[c]] if c in third else [])
        m1 += [k * 1_000_000 + 500 for k in keys]
        clip += [c] * len(keys)
    m1 = np.array(m1, np.int32)
    m2 = np.zeros(len(m1), np.int32)
    engine.index_clear()
    engine.index_add_batch(uuids, np.concatenate([[0], np.cumsum(np.bincount(clip))]), m1, m2)
    engine.index_set_scope(uuids, [c % 2 for c in range(C_)])
    p = tfp_lib.params(1, 0.001)
    clip = np.array(clip)
    best = {}
    for q1 in ([10.2, 11.2, 12.2], [10.2, 11.2, 13.2]):
        q2 = [0.0] * 3
        fr = R.frames_from_q(q1, q2)
        glob = R.brute_force(oracle, uuids, clip, m1, m2, q1, q2, 1, 0.001, -1, -1)
        for x in (0, 1):
            keep = clip % 2 == x
            exp = R.brute_force(oracle, uuids, clip[keep], m1[keep], m2[keep], q1, q2, 1, 0.001, -1, -1)
            assert len(exp) == C_ // 2 and exp[0][1] == 3 and exp[3][1] == exp[4][1] == 2  # ties inside the scope
            for k in (1, 8, 32):
                assert _scoped(engine, [fr], p, [x], k)[0] == exp[:k], (q1, x, k)
            best[(q1[2], x)] = uuids.index(exp[0][0])
        assert R.pairs(engine.search_ranked(fr, p, 8)) == glob[:8]
        assert _scoped(engine, [fr], p, [ANY], 32)[0] == glob[:32]
    # each scope's best: chunk 0 for one query, chunk 1 for the other; the global winner (1026, 1029) in the other scope
    assert best == {(12.2, 1): 1023, (12.2, 0): 1026, (13.2, 0): 4, (13.2, 1): 1029}
    engine.index_clear()


def test_general_form_and_scratch_restored(tfp_lib, oracle, monkeypatch):
    monkeypatch.setenv("TFP_WIDE_MIN_TOL", "1e9")  # plain general-path searches take the cells form / row scan
    scen, ranked = R.load_cases()
    scoped = S.load_scoped()
    name = "rand_05"
    s = scen[name]
    with tfp_lib.Engine(0) as eng:
        S.enrol_scoped(eng, s)
        c2 = [qi for qi, q in enumerate(s["queries"]) if q["coefs"] == 2]
        assert sum(bool(scoped[(name, qi)][x]) for qi in c2 for x in range(3)) > 3

        def plain_and_ranked():
            out = []
            for qi in c2:
                q = s["queries"][qi]
                fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
                out.append((eng.search_batch(fr, [0, len(fr)], p), eng.search_ranked_batch(fr, [0, len(fr)], p, 8)))
            return out

        before = plain_and_ranked()
        st0 = eng.scope_stats()
        for qi in c2:
            q = s["queries"][qi]
            fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
            assert _scoped(eng, [fr] * 4, p, [0, 1, 2, ANY], 8) == list(scoped[(name, qi)]) + [ranked[(name, qi)]], qi
        st1 = eng.scope_stats()
        assert (st1["vote_batches"], st1["general_batches"]) == (st0["vote_batches"], st0["general_batches"] + len(c2))
        # every touched clip's scratch, in scope or not, is zero again
        assert plain_and_ranked() == before
        qi = next(i for i, q in enumerate(s["queries"]) if q["coefs"] == 1 and q["tol"] == 0.001 and ranked[(name, i)])
        q = s["queries"][qi]
        assert _scoped(eng, [R.frames_from_q(q["q1"], q["q2"])], _params(tfp_lib, q), [1], 8)[0] == scoped[(name, qi)][1]
        st2 = eng.scope_stats()
        assert (st2["vote_batches"], st2["general_batches"]) == (st1["vote_batches"] + 1, st1["general_batches"])
        # coefs = 1 with a 600.0 dB query frame: a key outside the vote range, served by the general form
        uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(3)]
        m1 = [600_000_100, 24_000_000, 600_000_200, 24_000_100, 24_000_200]
        clip = [0, 0, 1, 2, 2]
        eng.index_clear()
        for c in range(3):
            eng.index_add(uuids[c], np.array([m for m, k in zip(m1, clip) if k == c], np.int32),
                          np.zeros(clip.count(c), np.int32))
        eng.index_set_scope(uuids, [5, 6, 5])
        q1, q2 = [600.0, 24.5, 24.7], [0.0, 0.0, 0.0]
        fr, p = R.frames_from_q(q1, q2), tfp_lib.params(1, 0.001)
        exp = R.brute_force(oracle, uuids, clip, m1, [0] * 5, q1, q2, 1, 0.001, -1, -1)
        assert exp == [(uuids[0], 3), (uuids[2], 2), (uuids[1], 1)]
        plain0 = (eng.search_batch(fr, [0, 3], p), eng.search_ranked_batch(fr, [0, 3], p, 8))
        assert R.pairs(plain0[1][0]) == exp
        assert _scoped(eng, [fr] * 3, p, [5, 6, 0], 8) == [[exp[0], exp[1]], [exp[2]], []]
        st3 = eng.scope_stats()
        assert (st3["vote_batches"], st3["general_batches"]) == (st2["vote_batches"], st2["general_batches"] + 1)
        assert (eng.search_batch(fr, [0, 3], p), eng.search_ranked_batch(fr, [0, 3], p, 8)) == plain0


@pytest.mark.parametrize("delta", ["1", "0"])
def test_index_delta(tfp_lib, monkeypatch, delta):
    monkeypatch.setenv("TFP_INDEX_DELTA", delta)  # 1: the delta at any index size; 0: every update merges
    scen, _ = R.load_cases()
    scoped = S.load_scoped()
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
        eng.search_scoped_batch(R.frames_from_q([24.3], [1.0]), [0, 1], tfp_lib.params(1, 0.001), [0], 1)
        for c in range(nc - 3, nc):  # enrolled after the build, scoped after enrolment
            eng.index_add(s["uuids"][c], m1[clip == c], m2[clip == c])
            eng.index_set_scope([s["uuids"][c]], [c % 3])
        in_delta = 3 if delta == "1" else 0
        n = {1: 0, 2: 0}
        for coefs in (1, 2):  # (coefs = 2 merges the delta: after the coefs = 1 queries)
            for qi, q in enumerate(s["queries"]):
                if q["coefs"] != coefs or q["tol"] != q["tol"] or q["tol"] > 8:
                    continue
                fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
                assert _scoped(eng, [fr] * 3, p, [0, 1, 2], 8) == list(scoped[(name, qi)]), (coefs, qi)
                n[coefs] += any(scoped[(name, qi)])
                if coefs == 1:
                    assert eng.index_delta_stats()[1] == in_delta  # served beside the index, not merged
        assert n[1] > 3 and n[2] > 0
        new = s["uuids"][nc - 3:]
        hit = [u for (nm, qi), per in scoped.items() if nm == name for rows in per for u, _ in rows if u in new]
        assert hit  # the clips enrolled after the build are among the expected rows


def test_scope_moves_and_table_builds(tfp_lib, oracle):
    scen, _ = R.load_cases()
    scoped = S.load_scoped()
    name = "rand_05"
    s = scen[name]
    qi = max((i for i, q in enumerate(s["queries"]) if q["coefs"] == 1 and q["tol"] == q["tol"] and q["tol"] <= 8),
             key=lambda i: min(len(rows) for rows in scoped[(name, i)]))
    q = s["queries"][qi]
    assert all(len(rows) >= 2 for rows in scoped[(name, qi)])
    fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
    uuids = list(s["uuids"])
    scope = {u: c % 3 for c, u in enumerate(uuids)}
    clip, m1, m2 = np.asarray(s["clip"], np.int64), np.asarray(s["m1"], np.int64), np.asarray(s["m2"], np.int64)

    def expect(x):
        keep = np.array([u in scope and scope[u] == x for u in uuids])[clip]
        return R.brute_force(oracle, uuids, clip[keep], m1[keep], m2[keep], q["q1"], q["q2"], q["coefs"], q["tol"], q["low"],
                             q["high"], limit=8)

    with tfp_lib.Engine(0) as eng:
        S.enrol_scoped(eng, s)

        def check(builds):
            for _ in range(10):
                assert _scoped(eng, [fr] * 3, p, [0, 1, 2], 8) == [expect(0), expect(1), expect(2)]
                assert eng.scope_stats()["table_builds"] == builds

        b = eng.scope_stats()["table_builds"]
        assert [expect(x) for x in range(3)] == list(scoped[(name, qi)])
        check(b + 1)
        # scope 0's winner moves to scope 1
        mover = expect(0)[0][0]
        eng.index_set_scope([mover], [1])
        scope[mover] = 1
        assert eng.index_scope(mover) == 1 and mover in [u for u, _ in expect(1)]
        check(b + 2)
        eng.index_set_scope([mover], [1])  # no change: no build
        check(b + 2)
        # the clip whose uuid sorts first goes: every column renumbers
        first = min(scope)
        eng.index_remove(first)
        del scope[first]
        check(b + 3)
        with pytest.raises(tfp_lib.TfpError) as err:
            eng.index_scope(first)
        assert err.value.code == TFP_E_NOENT
        # staging compaction: a 70,000-row clip enrolled and removed leaves more dead rows than it tolerates
        big = "ffffffff-0000-4000-8000-000000000000"
        eng.index_add(big, np.full(70_000, 900_000_000, np.int32), np.zeros(70_000, np.int32))
        eng.index_set_scope([big], [2])
        eng.index_commit()
        eng.index_remove(big)
        full0 = eng.index_build_stats()[0]
        check(b + 4)
        assert eng.index_build_stats()[0] == full0 + 1  # the update that compacted was a full build
        # a clip enrolled again under a removed uuid starts in scope 0
        c = uuids.index(first)
        eng.index_add(first, m1[clip == c].astype(np.int32), m2[clip == c].astype(np.int32))
        assert eng.index_scope(first) == 0
        scope[first] = 0
        check(b + 5)
        eng.index_clear()
        assert _scoped(eng, [fr], p, [0], 8) == [[]]


def test_arguments(engine, tfp_lib):
    from tiresias_amd._lib import Candidate
    scen, _ = R.load_cases()
    scoped = S.load_scoped()
    name = "rand_05"
    s = scen[name]
    S.enrol_scoped(engine, s)
    qi = next(i for i, q in enumerate(s["queries"]) if q["coefs"] == 1 and scoped[(name, i)][0])
    q = s["queries"][qi]
    fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
    L = tfp_lib.lib()

    def raw(scope, k, cap=40):
        out, cnt = (Candidate * cap)(), C.c_int32(-7)
        C.memset(out, 0xFF, C.sizeof(out))
        qoff, sc = (C.c_int64 * 2)(0, len(fr)), (C.c_int32 * 1)(scope)
        rc = L.tfp_search_scoped_batch(engine.handle, fr.ctypes.data, qoff, 1, C.byref(p), sc, k, out, C.byref(cnt))
        return rc, out, cnt.value

    for scope, k in ((-2, 4), (-100, 4), (0, 0), (0, 33), (0, -1)):
        assert raw(scope, k)[0] == TFP_E_ARG, (scope, k)
    rc, out, cnt = raw(0, 8, cap=8)
    exp = scoped[(name, qi)][0]
    assert rc == 0 and cnt == len(exp) and [(c.uuid.decode(), c.match_count) for c in out[:cnt]] == exp
    assert bytes(out)[cnt * C.sizeof(out[0]):] == bytes((8 - cnt) * C.sizeof(out[0]))  # zeroed past counts[q]
    rc, out, cnt = raw(S.UNUSED_SCOPE, 8, cap=8)
    assert rc == 0 and cnt == 0 and bytes(out) == bytes(C.sizeof(out))
    # set_scope is all or nothing
    a, b = s["uuids"][0], s["uuids"][1]
    was = (engine.index_scope(a), engine.index_scope(b))
    for uu, sc, code in (([a, b], [5, -1], TFP_E_ARG), ([a, "no-such-uuid", b], [5, 5, 5], TFP_E_NOENT)):
        with pytest.raises(tfp_lib.TfpError) as err:
            engine.index_set_scope(uu, sc)
        assert err.value.code == code
        assert (engine.index_scope(a), engine.index_scope(b)) == was
    assert _scoped(engine, [fr], p, [0], 8)[0] == exp
    v, g, t = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.tfp_scope_stats(engine.handle, None, None, None) == 0
    assert L.tfp_scope_stats(engine.handle, C.byref(v), None, C.byref(t)) == 0 and v.value > 0 and t.value > 0
    assert L.tfp_scope_stats(engine.handle, None, C.byref(g), None) == 0 and g.value >= 0
    engine.index_clear()
    rc, out, cnt = raw(0, 8, cap=8)  # an empty index
    assert rc == 0 and cnt == 0 and bytes(out) == bytes(C.sizeof(out))
    assert engine.search_scoped_batch(R.frames_from_q([], []), [0], p, [], 4) == []  # no query


def test_same_rows_under_two_uuids_in_two_scopes(engine, tfp_lib):
    """The catalog's MD5 dedup is per context: one file in two contexts is two clips with identical rows."""
    lo, hi = "11111111-0000-4000-8000-000000000000", "99999999-0000-4000-8000-000000000000"
    other = "55555555-0000-4000-8000-000000000000"
    m1 = np.array([24_000_100, 30_000_100, 36_000_100], np.int32)
    engine.index_clear()
    for u, rows in ((hi, m1), (lo, m1), (other, m1[:1])):
        engine.index_add(u, rows, np.zeros(len(rows), np.int32))
    engine.index_set_scope([lo, hi, other], [1, 2, 1])
    fr, p = R.frames_from_q([24.5, 30.5, 36.5], [0.0] * 3), tfp_lib.params(1, 0.001)
    plain, _ = engine.search(fr, p)
    assert (plain["audio_uuid"], plain["match_count"]) == (hi, 3)  # unscoped: the greater uuid of the tie
    assert _scoped(engine, [fr] * 3, p, [1, 2, ANY], 8) == [[(lo, 3), (other, 1)], [(hi, 3)], [(hi, 3), (lo, 3), (other, 1)]]
    engine.index_clear()


def test_group_of_three_equals_one_engine(engine, tfp_lib):
    scen, _ = R.load_cases()
    scoped = S.load_scoped()
    g = tfp_lib.Group([0, 0, 0])
    try:
        for name in ("rand_05", "tie_2000"):
            s = scen[name]
            S.enrol_scoped(engine, s)
            S.enrol_scoped(g, s)
            assert [g.index_scope(u) for u in s["uuids"][:7]] == [c % 3 for c in range(7)]
            if name == "tie_2000":
                # equal clips land on the shards in turn, so scope c % 3 lies on one shard: scopes by
                # c // 3 % 3 instead spread each scope's tied clips over all three
                for e in (engine, g):
                    e.index_set_scope(s["uuids"], [c // 3 % 3 for c in range(len(s["uuids"]))])
            kinds = [0, 1, 2, ANY, S.UNUSED_SCOPE]
            for qis in _by_params(s).values():
                p = _params(tfp_lib, s["queries"][qis[0]])
                frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in kinds]
                fr, qoff = _batch(frames)
                got = g.search_scoped_batch(fr, qoff, p, kinds * len(qis), 8)
                assert [R.pairs(r) for r in got] == _scoped(engine, frames, p, kinds * len(qis), 8), name
                for j, i in enumerate(qis):
                    if name != "tie_2000":
                        assert [R.pairs(r) for r in got[j * 5:j * 5 + 3]] == list(scoped[(name, i)]), (name, i)
            if name == "tie_2000":  # ties inside one scope, across shards
                rows = [r for r in got[:3] if r]
                assert rows and all(len({c["match_count"] for c in r}) == 1 and len({c["clip_id"] for c in r}) > 1
                                    for r in rows)
        with pytest.raises(tfp_lib.TfpError) as err:
            g.index_set_scope([s["uuids"][0], "no-such-uuid"], [4, 4])
        assert err.value.code == TFP_E_NOENT and g.index_scope(s["uuids"][0]) == 0
        st = g.scope_stats()
        assert st["vote_batches"] > 0 and st["table_builds"] >= 3
    finally:
        g.close()
        engine.index_clear()


def test_pcm_form_equals_frames_form(engine, tfp_lib):
    n = 8000 * 5
    pcm = tfp_lib.synth_pcm(0x7153A1, range(2), n)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(3) * n)
    nf = len(fr) // 2
    uuids = ["00000000-0000-4000-8000-00000000000%d" % i for i in range(2)]
    engine.index_clear()
    for c in range(2):
        engine.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    engine.index_set_scope(uuids, [3, 4])
    q = np.ascontiguousarray(pcm[:, :16000]).reshape(-1)
    off = np.arange(3) * 16000
    qfr = engine.fingerprint_batch(q, off)
    qoff = np.arange(3) * (len(qfr) // 2)
    seen = 0
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(2, 0.45)):
        for scopes in ([3, 4], [4, ANY], [0, 3]):
            got = engine.search_scoped_pcm_batch(q, off, p, scopes, 2)
            assert got == engine.search_scoped_batch(qfr, qoff, p, scopes, 2)
            ranked = engine.search_ranked_batch(qfr, qoff, p, 2)
            for i, x in enumerate(scopes):
                want = [r for r in ranked[i] if x == ANY or r["audio_uuid"] == dict(zip([3, 4], uuids)).get(x)]
                assert got[i] == want, (p.coefs, scopes, i)
                seen += len(want)
    assert seen > 0
    engine.index_clear()


def test_fp_handler_in_context(tmp_path, tfp_lib):
    """12 clips in two contexts, as the mirror's end-to-end test builds them: the in-context search
    returns fp_search_fingerprint_candidates' rows of that context, in their order."""
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    fp = FpHandler(0, backup_path=str(tmp_path / "snap.db"))
    assert fp.fp_init()
    pcm = tfp_lib.synth_pcm(0x7153A1, range(12), 8000 * 8)
    for i in range(12):
        f = str(tmp_path / f"clip{i}.wav")
        write_wav_mono16(f, pcm[i])
        assert fp.fp_craete_audio_list_info("ctx%d" % (i % 2), f)
    # clip 5's file once more, in the other context: a second clip with identical rows
    assert fp.fp_craete_audio_list_info("ctx0", str(tmp_path / "clip5.wav"))
    assert len(fp.fp_get_audio_lists_all()) == 13
    q = str(tmp_path / "q.wav")
    write_wav_mono16(q, pcm[5][256 * 40: 256 * 40 + 24000])

    def checks(fp):
        every = fp.fp_search_fingerprint_candidates("ctx1", q, 1, 0.45, -1, -1, 32)
        assert len(every) >= 2 and {r["context"] for r in every} == {"ctx0", "ctx1"}
        five = [r for r in every if r["name"] == "clip5.wav"]  # the two enrolments of clip 5: one per context, tied
        assert sorted(r["context"] for r in five) == ["ctx0", "ctx1"] and five[0]["match_count"] == five[1]["match_count"]
        assert five[0]["uuid"] > five[1]["uuid"]
        for ctx in ("ctx0", "ctx1"):
            mine = [r for r in every if r["context"] == ctx]
            assert fp.fp_search_fingerprint_in_context(ctx, q, 1, 0.45, -1, -1, 32) == mine
            assert fp.fp_search_fingerprint_in_context(ctx, q, 1, 0.45, -1, -1) == mine[:1]
            assert [r["name"] for r in mine].count("clip5.wav") == 1 and mine[0]["frame_count"] == 94
            assert fp.fp_search_fingerprint_in_context(ctx, q, 2, 0.45, -1, -1, 32) == \
                [r for r in fp.fp_search_fingerprint_candidates(ctx, q, 2, 0.45, -1, -1, 32) if r["context"] == ctx]
        assert fp.fp_search_fingerprint_in_context("nowhere", q, 1, 0.45, -1, -1, 32) == []
        assert fp.fp_search_fingerprint_in_context("ctx1", q, 3, 0.45, -1, -1, 32) == []
        assert fp.fp_search_fingerprint_in_context("ctx1", str(tmp_path / "missing.wav"), 1, 0.45, -1, -1, 32) == []
        return every

    before = checks(fp)
    assert fp.fp_term()
    again = FpHandler(0, backup_path=str(tmp_path / "snap.db"))  # the scopes come back from audio_list's contexts
    assert again.fp_init()
    assert checks(again) == before
    assert again.fp_term()
