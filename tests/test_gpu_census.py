"""Match census (tfp_census*, csrc/tfp_census.hip): per query the exact number of clips of the query's
scope at each count(*) of the reference's result query (fp_handler.c:367-374), against the
SQLite-peeled fixture tests/golden/census_cases.json and a brute-force count grouped by scope."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import census_util as U
import ranked_util as R
import scoped_util as S

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
ANY = U.ANY
KINDS = [ANY, 0, 1, 2, S.UNUSED_SCOPE]


def _lds_bins():
    with open(os.path.join(R.REPO, "asterisk-tiresias_amd", "csrc", "tfp_census.hpp")) as f:
        return int(re.search(r"constexpr int32_t kCensusLdsBins = (\d+);", f.read()).group(1))


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _batch(frames):
    return np.concatenate(frames), np.concatenate([[0], np.cumsum([len(f) for f in frames])])


def _uuids(n):
    return ["00000000-0000-4000-8000-%012d" % c for c in range(n)]


def _enrol(eng, uuids, keys_of, scopes=None):
    """Clip c with one row per key of keys_of(c) (max1 = key dB + 500 micro); returns (clip, m1, m2)."""
    clip, m1 = [], []
    for c in range(len(uuids)):
        ks = keys_of(c)
        m1 += [R.NULL if k is None else k * 1_000_000 + 500 for k in ks]
        clip += [c] * len(ks)
    m1, m2 = np.array(m1, np.int64).astype(np.int32), np.zeros(len(m1), np.int32)
    eng.index_clear()
    eng.index_add_batch(uuids, np.concatenate([[0], np.cumsum(np.bincount(clip, minlength=len(uuids)))]), m1, m2)
    if scopes is not None:
        eng.index_set_scope(uuids, scopes)
    return np.array(clip, np.int64), m1, m2


def _raw(tfp_lib, eng, fr, qoff, p, scopes, nbins, fill=-77):
    """tfp_census_batch through ctypes with hist pre-filled: (rc, hist [nq, nbins], need_bins)."""
    nq = len(qoff) - 1
    hist = np.full((max(nq, 1), max(nbins, 1)), fill, np.int32)
    need = C.c_int32(-9)
    qo = np.ascontiguousarray(qoff, np.int64)
    sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
    rc = tfp_lib.lib().tfp_census_batch(eng.handle, fr.ctypes.data, qo.ctypes.data, nq, C.byref(p),
                                        None if sc is None else sc.ctypes.data, nbins, hist.ctypes.data, C.byref(need))
    return rc, hist, need.value


def test_goldens_every_query_any_each_context_and_a_scope_nobody_has(engine, tfp_lib):
    scen, _ = R.load_cases()
    census = U.load_census()
    n = 0
    for name, s in scen.items():
        S.enrol_scoped(engine, s)
        by_p = {}
        for qi, q in enumerate(s["queries"]):
            if q["coefs"] in (1, 2):
                by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
        for qis in by_p.values():  # the queries of one parameter set, each in the five scopes, as one batch
            p = _params(tfp_lib, s["queries"][qis[0]])
            frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in KINDS]
            fr, qoff = _batch(frames)
            got = engine.census_batch(fr, qoff, p, KINDS * len(qis))
            nbins = max(len(f) for f in frames) + 1
            assert got.shape == (len(frames), nbins) and got.dtype == np.int32
            for j, i in enumerate(qis):
                for t, x in enumerate(KINDS):
                    cen = () if x == S.UNUSED_SCOPE else census[(name, i)][0 if x == ANY else 1 + x]
                    exp = U.dense(cen, U.scenario_population(s, x), nbins)  # row for row, bin 0 included
                    assert np.array_equal(got[j * len(KINDS) + t], exp), (name, i, x)
                    n += 1
        if name == "tie_2000":  # 2,000 equal counts in two column chunks: the aggregated adds, the cross-block flush
            assert max(got[0]) == 2000 and engine.census_stats()["vote_batches"] > 0
    engine.index_clear()
    assert n > 5 * 850


@pytest.mark.parametrize("ncols", [1, 3, 1023, 1024, 1025, 2050])
def test_column_edges(engine, tfp_lib, oracle, ncols):
    """Clips of 2-4 rows: padding columns of the scope table, a column count that is no multiple of 4,
    more than two blocks."""
    uuids = _uuids(ncols)
    scopes = [c % 2 for c in range(ncols)]
    clip, m1, m2 = _enrol(engine, uuids, lambda c: [10, 11] + [12] * (c % 3 == 1) + [13] * (c % 5 == 2), scopes)
    assert set(np.bincount(clip)) <= {2, 3, 4}
    q1s = ([10.2, 11.2, 12.2, 13.2, 50.2], [12.2, 13.2, 13.3], [11.2])
    frames = [R.frames_from_q(q1, [0.0] * len(q1)) for q1 in q1s for _ in (ANY, 0, 1)]
    fr, qoff = _batch(frames)
    p = tfp_lib.params(1, 0.001)
    got = engine.census_batch(fr, qoff, p, [ANY, 0, 1] * len(q1s))
    scope_of = dict(zip(uuids, scopes))
    for j, q1 in enumerate(q1s):
        rows = R.brute_force(oracle, uuids, clip, m1, m2, q1, [0.0] * len(q1), 1, 0.001, -1, -1)
        for t, x in enumerate((ANY, 0, 1)):
            exp = U.brute_census(oracle, uuids, scope_of, clip, m1, m2, q1, [0.0] * len(q1), 1, 0.001, -1, -1, x, got.shape[1])
            row = got[j * 3 + t]
            assert np.array_equal(row, exp), (ncols, q1, x)
            hit = sum(1 for u, _ in rows if x == ANY or scope_of[u] == x)
            assert row[1:].sum() == hit == tfp_lib.census_at_least(row, 1)  # bins >= 1: the clips with a hit
            assert row.sum() == sum(1 for c in range(ncols) if x == ANY or scopes[c] == x)  # bin 0 closes to the population
    assert got[0][2:].sum() == ncols  # (every clip has both rows of the first query's keys 10 and 11)
    engine.index_clear()


def test_count_edges(engine, tfp_lib, oracle):
    """A clip every frame hits, a query without frames, a query whose frames the filters ignore, NULL
    max1 rows, a row-less clip (bin 0) and a removed clip (no bin)."""
    uuids = _uuids(6)
    keys = {0: [20, 21, 22, 23], 1: [20, None, None], 2: [None, None], 3: [], 4: [20, 21], 5: [21]}
    scopes = [1, 1, 1, 1, 2, 2]
    clip, m1, m2 = _enrol(engine, uuids, lambda c: keys[c], scopes)
    engine.index_remove(uuids[4])
    live = [u for u in uuids if u != uuids[4]]
    keep = clip != 4
    lclip = np.array([live.index(uuids[c]) for c in clip[keep]], np.int64)
    scope_of = dict(zip(uuids, scopes))
    q1s = ([20.2, 21.2, 22.2, 23.2, 20.3, 21.3], [], [20.2], [55.5, 56.5])
    frames = [R.frames_from_q(q1, [0.0] * len(q1)) for q1 in q1s for _ in (ANY, 1, 2)]
    fr, qoff = _batch(frames)
    for p, lo in ((tfp_lib.params(1, 0.001), -1), (tfp_lib.params(1, 0.001, 1_000_000, -1), 1_000_000)):
        got = engine.census_batch(fr, qoff, p, [ANY, 1, 2] * len(q1s))
        assert got.shape == (3 * len(q1s), 7)
        for j, q1 in enumerate(q1s):
            for t, x in enumerate((ANY, 1, 2)):
                exp = U.brute_census(oracle, live, scope_of, lclip, m1[keep], m2[keep], q1, [0.0] * len(q1), 1, 0.001, lo,
                                     -1, x, 7)
                assert np.array_equal(got[j * 3 + t], exp), (lo, q1, x)
        if lo < 0:
            assert list(got[0]) == [2, 0, 2, 0, 0, 0, 1]  # ANY: clip 0 in bin F = 6; the NULL-only and row-less clips in bin 0
            assert list(got[1]) == [2, 0, 1, 0, 0, 0, 1] and list(got[2]) == [0, 0, 1, 0, 0, 0, 0]  # (the removed clip 4: nowhere)
            assert list(got[3]) == [5, 0, 0, 0, 0, 0, 0]  # F = 0: every live clip in bin 0
        else:  # 10 log10(10^6) = 60 dB: every frame below it is ignored
            assert [list(r) for r in got] == [[5, 0, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0]] * len(q1s)
    # a batch of queries without a frame, and the clip-less index
    none = R.frames_from_q([], [])
    assert engine.census_batch(none, [0, 0, 0], tfp_lib.params(1, 0.001), [ANY, 2]).tolist() == [[5], [1]]
    engine.index_clear()
    assert not engine.census_batch(fr, qoff, tfp_lib.params(1, 0.001), [ANY, 1, 2] * len(q1s)).any()
    assert not engine.census_batch(fr, qoff, tfp_lib.params(2, 0.45), None).any()


def test_lds_bin_boundary_and_capacity(engine, tfp_lib, oracle):
    """Queries of kCensusLdsBins - 1, kCensusLdsBins and kCensusLdsBins + 1 frames against 1,030 clips: one
    clip (in the second column chunk) hit by every frame, the others by one."""
    B = _lds_bins()
    ncols, star = 1030, 1027
    uuids = _uuids(ncols)
    scopes = [c % 2 for c in range(ncols)]
    clip, m1, m2 = _enrol(engine, uuids, lambda c: [10, 11] if c == star else [11], scopes)
    scope_of = dict(zip(uuids, scopes))
    p = tfp_lib.params(1, 0.001)
    lens = [B - 1, B, B + 1]
    frames = [R.frames_from_q([10.2] * (F - 1) + [11.2], [0.0] * F) for F in lens for _ in (ANY, 0, 1)]
    fr, qoff = _batch(frames)
    kinds = [ANY, 0, 1] * len(lens)
    rc, got, need = _raw(tfp_lib, engine, fr, qoff, p, kinds, B + 2)
    assert rc == 0 and need == B + 2
    for j, F in enumerate(lens):
        q1 = [10.2] * (F - 1) + [11.2]
        for t, x in enumerate((ANY, 0, 1)):
            exp = U.brute_census(oracle, uuids, scope_of, clip, m1, m2, q1, [0.0] * F, 1, 0.001, -1, -1, x, B + 2)
            assert np.array_equal(got[j * 3 + t], exp), (F, x)
        assert got[j * 3][F] == 1 and got[j * 3][1] == ncols - 1 and got[j * 3].sum() == ncols
        assert got[j * 3 + 1 + star % 2][F] == 1 and got[j * 3 + 2 - star % 2][F] == 0
    # one bin short: TFP_E_CAPACITY, need_bins set, hist untouched
    rc, hist, need = _raw(tfp_lib, engine, fr, qoff, p, kinds, B + 1, fill=-77)
    assert rc == TFP_E_CAPACITY and need == B + 2 and (hist == -77).all()
    with pytest.raises(tfp_lib.TfpError) as err:
        engine.census_batch(fr, qoff, p, kinds, nbins=B + 1)
    assert err.value.code == TFP_E_CAPACITY
    # more bins than needed: the bins past the query's frames are zero
    wide = engine.census_batch(fr, qoff, p, kinds, nbins=B + 40)
    assert np.array_equal(wide[:, :B + 2], got) and not wide[:, B + 2:].any()
    engine.index_clear()


def test_forms(tfp_lib, oracle):
    """coefs = 2 and a coefs = 1 key outside the vote range take the general form; both forms agree with
    brute force, and with each other on queries both can serve; the scan scratch is restored."""
    scen, ranked = R.load_cases()
    s = scen["rand_05"]
    scope_of = {u: c % 3 for c, u in enumerate(s["uuids"])}
    with tfp_lib.Engine(0) as eng:
        S.enrol_scoped(eng, s)
        st = eng.census_stats()
        assert st == {"vote_batches": 0, "general_batches": 0}
        seen = 0
        for tol in (0.001, 0.45):
            for qi, q in enumerate([q for q in s["queries"] if q["q1"]][:12]):  # (a batch without a frame launches nothing)
                fr, p = R.frames_from_q(q["q1"], q["q2"]), tfp_lib.params(2, tol, q["low"], q["high"])
                before = eng.search_ranked_batch(fr, [0, len(fr)], p, 8)
                got = eng.census_batch(np.concatenate([fr] * 4), np.arange(5) * len(fr), p, [ANY, 0, 1, 2])
                for t, x in enumerate((ANY, 0, 1, 2)):
                    exp = U.brute_census(oracle, s["uuids"], scope_of, s["clip"], s["m1"], s["m2"], q["q1"], q["q2"], 2, tol,
                                         q["low"], q["high"], x, len(fr) + 1)
                    assert np.array_equal(got[t], exp), (tol, qi, x)
                seen += int(got[0][1:].sum())
                st["general_batches"] += 1
                assert eng.census_stats() == st
                assert eng.search_ranked_batch(fr, [0, len(fr)], p, 8) == before  # every touched clip's scratch is zero again
        assert seen > 0
        # coefs = 1: the vote form; with a 600.0 dB frame in the batch, the general form, on the same queries
        c1 = [qi for qi, q in enumerate(s["queries"]) if q["coefs"] == 1 and q["tol"] == 0.001 and q["low"] == q["high"] == -1
              and ranked[("rand_05", qi)]][:6]
        assert len(c1) >= 3
        p = tfp_lib.params(1, 0.001)
        frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in c1 for _ in (ANY, 0, 1, 2)]
        kinds = [ANY, 0, 1, 2] * len(c1)
        fr, qoff = _batch(frames)
        nb = max(len(f) for f in frames) + 2
        vote = eng.census_batch(fr, qoff, p, kinds, nbins=nb)
        st["vote_batches"] += 1
        assert eng.census_stats() == st
        far = R.frames_from_q([600.0, 24.5], [0.0, 0.0])
        fr2, qoff2 = _batch(frames + [far])
        general = eng.census_batch(fr2, qoff2, p, kinds + [ANY], nbins=nb)
        st["general_batches"] += 1
        assert eng.census_stats() == st
        assert np.array_equal(general[:-1], vote) and vote[:, 1:].any()
        for j, i in enumerate(c1):
            q = s["queries"][i]
            for t, x in enumerate((ANY, 0, 1, 2)):
                exp = U.brute_census(oracle, s["uuids"], scope_of, s["clip"], s["m1"], s["m2"], q["q1"], q["q2"], 1, 0.001, -1,
                                     -1, x, nb)
                assert np.array_equal(vote[j * 4 + t], exp), (i, x)
        exp = U.brute_census(oracle, s["uuids"], scope_of, s["clip"], s["m1"], s["m2"], [600.0, 24.5], [0.0, 0.0], 1, 0.001,
                             -1, -1, ANY, nb)
        assert np.array_equal(general[-1], exp)
        # rows at 600 dB: the out-of-range key does hit
        uuids = _uuids(3)
        clip, m1, m2 = _enrol(eng, uuids, lambda c: [[600, 24], [600], [24, 24]][c], [5, 6, 5])
        q1 = [600.0, 24.5, 24.7]
        got = eng.census_batch(np.concatenate([R.frames_from_q(q1, [0.0] * 3)] * 3), [0, 3, 6, 9], p, [ANY, 5, 6])
        for t, x in enumerate((ANY, 5, 6)):
            exp = U.brute_census(oracle, uuids, dict(zip(uuids, [5, 6, 5])), clip, m1, m2, q1, [0.0] * 3, 1, 0.001, -1, -1, x, 4)
            assert np.array_equal(got[t], exp), x
        assert got.tolist() == [[0, 1, 1, 1], [0, 0, 1, 1], [0, 1, 0, 0]]
        st["general_batches"] += 1
        assert eng.census_stats() == st


def test_index_delta_and_scope_change(tfp_lib, oracle):
    """5 clips enrolled after a first search into a 4,100-column index lie in the index delta: the vote
    form serves them from the bitsets at a tolerance the delta's bits cover, and merges them first at
    one they do not; a scope changed between two calls is seen by the next."""
    n0, n1 = 4100, 5
    uuids = _uuids(n0 + n1)
    scopes = [c % 3 for c in range(n0 + n1)]
    keys_of = lambda c: [10 + c % 7, 30] + [31] * (c % 11 == 0)  # noqa: E731
    with tfp_lib.Engine(0) as eng:
        clip, m1, m2 = _enrol(eng, uuids[:n0], keys_of, scopes[:n0])
        eng.index_commit()
        q1 = [10.2, 12.2, 30.2, 31.2, 16.4]
        fr = R.frames_from_q(q1, [0.0] * len(q1))
        frs, qoff = np.concatenate([fr] * 4), np.arange(5) * len(fr)
        eng.census_batch(frs, qoff, tfp_lib.params(1, 0.001), [ANY, 0, 1, 2])
        for c in range(n0, n0 + n1):  # (uuids that sort after every indexed one and, for the last, before)
            u = uuids[c] if c < n0 + n1 - 1 else "00000000-0000-4000-7000-000000000000"
            uuids[c] = u
            eng.index_add(u, np.array([k * 1_000_000 + 500 for k in keys_of(c)], np.int32), np.zeros(len(keys_of(c)), np.int32))
            eng.index_set_scope([u], [scopes[c]])
        clip2, m1b, _ = _rows(n0, n1, keys_of)
        clip, m1, m2 = np.concatenate([clip, clip2]), np.concatenate([m1, m1b]), np.zeros(len(m1) + len(m1b), np.int32)
        scope_of = dict(zip(uuids, scopes))

        def check(tol, in_delta):
            got = eng.census_batch(frs, qoff, tfp_lib.params(1, tol), [ANY, 0, 1, 2])
            assert eng.index_delta_stats()[1] == in_delta
            for t, x in enumerate((ANY, 0, 1, 2)):
                exp = U.brute_census(oracle, uuids, scope_of, clip, m1, m2, q1, [0.0] * len(q1), 1, tol, -1, -1, x, len(q1) + 1)
                assert np.array_equal(got[t], exp), (tol, x)
            return got

        a = check(0.001, n1)  # served beside the index, not merged
        assert a[0].sum() == n0 + n1
        mover = uuids[n0 + 1]  # a delta clip changes scope: the next census sees it
        eng.index_set_scope([mover], [(scope_of[mover] + 1) % 3])
        scope_of[mover] = (scope_of[mover] + 1) % 3
        b = check(0.001, n1)
        assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1:], b[1:])
        check(9.0, 0)  # a tolerance the delta's bits do not cover: merged first
        mover = uuids[7]
        eng.index_set_scope([mover], [(scope_of[mover] + 1) % 3])
        scope_of[mover] = (scope_of[mover] + 1) % 3
        c = check(0.001, 0)
        assert not np.array_equal(b[1:], c[1:])
        st = eng.census_stats()
        assert st["vote_batches"] == 5 and st["general_batches"] == 0


def _rows(first, n, keys_of):
    clip, m1 = [], []
    for c in range(first, first + n):
        for k in keys_of(c):
            clip.append(c)
            m1.append(k * 1_000_000 + 500)
    return np.array(clip, np.int64), np.array(m1, np.int32), None


def test_consistent_with_scoped_search(engine, tfp_lib):
    """On one batch: the counts of tfp_search_scoped_batch's 32 rows are the census read from the top,
    and the rows with count >= c number min(32, tfp_census_at_least(c))."""
    scen, _ = R.load_cases()
    checked = 0
    for name in ("tie_2000", "rand_05"):
        s = scen[name]
        S.enrol_scoped(engine, s)
        qis = [i for i, q in enumerate(s["queries"]) if q["coefs"] == 1 and q["tol"] == 0.001 and q["low"] == q["high"] == -1]
        assert qis
        frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in KINDS]
        fr, qoff = _batch(frames)
        p = tfp_lib.params(1, 0.001)
        rows = engine.search_scoped_batch(fr, qoff, p, KINDS * len(qis), 32)
        hist = engine.census_batch(fr, qoff, p, KINDS * len(qis))
        for got, row in zip(rows, hist):
            counts = [r["match_count"] for r in got]
            top = [c for c in range(len(row) - 1, 0, -1) for _ in range(row[c])]
            assert counts == top[:32]
            for c in range(1, len(row) + 1):
                assert sum(1 for n in counts if n >= c) == min(32, tfp_lib.census_at_least(row, c))
            checked += len(counts)
    assert checked > 32 * 4
    engine.index_clear()


def test_pcm_form_equals_frames_form(engine, tfp_lib):
    n = 8000 * 5
    pcm = tfp_lib.synth_pcm(0x7153A1, range(4), n)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(5) * n)
    nf = len(fr) // 4
    uuids = _uuids(4)
    engine.index_clear()
    for c in range(4):
        engine.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    engine.index_set_scope(uuids, [3, 4, 3, 4])
    q = np.concatenate([pcm[1, :24000], pcm[2, 4000:16000]])  # two queries of different lengths
    off = np.array([0, 24000, 36000])
    qfr = engine.fingerprint_batch(q, off)
    qoff = np.array([0, tfp_lib.frame_count(24000), tfp_lib.frame_count(24000) + tfp_lib.frame_count(12000)])
    assert qoff[2] == len(qfr) and qoff[1] != qoff[2] - qoff[1]
    seen = 0
    for p in (tfp_lib.params(1, 0.45), tfp_lib.params(1, 0.001), tfp_lib.params(2, 0.45)):
        for scopes in ([3, 4], [ANY, ANY], None, [0, 3]):
            got = engine.census_pcm_batch(q, off, p, scopes)
            assert got.shape == (2, tfp_lib.frame_count(24000) + 1)
            assert np.array_equal(got, engine.census_batch(qfr, qoff, p, scopes))
            seen += int(got[:, 1:].sum())
            assert got.sum(axis=1).tolist() == [{3: 2, 4: 2, ANY: 4, 0: 0}[x] for x in (scopes or [ANY, ANY])]
    assert seen > 0
    none = engine.census_pcm_batch(np.zeros(0, np.int16), [0, 0], tfp_lib.params(1, 0.45), [3])
    assert none.tolist() == [[2]]
    engine.index_clear()


def test_arguments(engine, tfp_lib):
    scen, _ = R.load_cases()
    s = scen["rand_05"]
    S.enrol_scoped(engine, s)
    q = s["queries"][0]
    fr, p = R.frames_from_q(q["q1"], q["q2"]), tfp_lib.params(1, 0.001)
    F = len(fr)
    L = tfp_lib.lib()
    rc, hist, need = _raw(tfp_lib, engine, fr, [0, F], p, [ANY], F + 1)
    assert rc == 0 and need == F + 1 and hist.sum() == len(s["uuids"])
    rc, none, _ = _raw(tfp_lib, engine, fr, [0, F], p, None, F + 1)  # scopes NULL: ANY
    assert rc == 0 and np.array_equal(none, hist)
    for scopes, params, qoff in (([-2], p, [0, F]), ([-100], p, [0, F]), ([0], tfp_lib.params(0, 0.001), [0, F]),
                                 ([0], tfp_lib.params(3, 0.001), [0, F]), ([0, 0], p, [0, F, F - 1])):
        rc, h, _ = _raw(tfp_lib, engine, fr, qoff, params, scopes, F + 1)
        assert rc == TFP_E_ARG and (h == -77).all(), (scopes, qoff)
    qo = (C.c_int64 * 2)(0, F)
    assert L.tfp_census_batch(engine.handle, fr.ctypes.data, qo, 1, C.byref(p), None, F + 1, hist.ctypes.data, None) == TFP_E_ARG
    rc, h, need = _raw(tfp_lib, engine, fr, [0], p, [], 1)  # no query
    assert rc == 0 and need == 1 and (h == -77).all()
    v, g = C.c_int64(-1), C.c_int64(-1)
    assert L.tfp_census_stats(engine.handle, None, None) == 0
    assert L.tfp_census_stats(engine.handle, C.byref(v), C.byref(g)) == 0 and v.value > 0 and g.value >= 0
    engine.index_clear()
