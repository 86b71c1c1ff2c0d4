"""Every search form at the tolerances where its path changes (tolerance_util.TOLS: 0, around the last digit
"%f" prints, kOrderMaxTol and the next printed value, 0.5, around 1, 1.5, the 8.0 of delta_tol_ok and the next
printed value, 600, around kKeyRange, past fmt6_bound's 1e12, 1e300, inf, nan), coefs 1 and 2, in three index
states, against the brute-force count over the oracle's boxes (tolerance_util.reference, pinned to SQLite by
tests/test_tolerance_oracle.py). Results are integers: every comparison is exact.

The states (one module-scoped engine each): "main", a full build of all 64 clips (TFP_INDEX_FULL); "delta",
52 clips built and the dozen of tolerance_util.DELTA added afterwards (TFP_INDEX_DELTA=1: delta columns);
"removed", the delta state after the removal of two of the delta's clips (the delta stays beside the main
index). Where a call merges the delta, it is put back before the next call.

A key outside the vote range is flagged for the whole batch and sends it to the general form over the sorted
rows (which merges a delta). So every form runs twice per tolerance: the 23 queries whose keys are all in range
in one batch (IN), and the query with the frame at 600.0 in a batch of its own (OUT); for the neighbours the
clips without a row past the key range, and clip 44 on its own. After every call (_call) the form's own counter
says which form served it and, with a delta, index_delta_stats whether the dozen clips are still in delta
columns: for coefs = 1 at the tolerances delta_tol_ok names, for the plain coefs = 2 sweep up to kOrderMaxTol,
and merged in every other case. search_aligned_batch and search_sliding_aligned_batch have no form counter of
their own (their counters count alignment work): with a delta its survival tells the form, in the main state
their results only. align_batch names its clips and searches nothing: its results only.

inf and nan: "%f" prints no SQL literal, no frame runs (fp_handler.c:357-359), and include/tiresias_fp.h names
no error for a tolerance: every form returns 0 with NOTFOUND or empty rows and the frames counted. That is the
reference's answer at those tolerances too, so the same comparisons cover it (a call that failed would raise)."""
import math
import os

import numpy as np
import pytest

import align_util as A
import census_util as CU
import live_util as L
import live_window_util as LW
import neighbour_util as N
import ranked_util as R
import tolerance_util as T

pytestmark = pytest.mark.gpu

K = 4
STATES = ("main", "delta", "removed")
Q_RANGE_OUT = 4  # the query with the frame at 600.0
NQ = 24
IN = tuple(i for i in range(NQ) if i != Q_RANGE_OUT)
OUT = (Q_RANGE_OUT,)


def _engine_with(tfp_lib, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tfp_lib.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class State:
    """An engine in one of the three states. extra: clips (uuid, m1, m2, scope) enrolled beside the tolerance
    index, after the delta's dozen (the live test's sources)."""

    def __init__(self, tfp_lib, name, extra=()):
        sp = T.spec()
        self.name = name
        self.eng = _engine_with(tfp_lib, {"TFP_INDEX_FULL": "1"} if name == "main" else {"TFP_INDEX_DELTA": "1"})
        clip = lambda c: (sp["uuids"][c], sp["clips"][c]["m1"], sp["clips"][c]["m2"], int(sp["scope"][c]))
        self.late = [clip(c) for c in T.DELTA] + list(extra)
        self.gone = [sp["uuids"][c] for c in T.REMOVED] if name == "removed" else []
        self.live = tuple(c for c in range(T.NCLIPS) if name != "removed" or c not in T.REMOVED)
        try:
            self._add([clip(c) for c in sp["order"]])
            if name != "main":
                self.eng.index_commit()
            self._late()
            self.dsize = self.eng.index_delta_stats()[1]
            assert self.dsize == (0 if name == "main" else len(self.late) - len(self.gone)), (name, self.dsize)
        except Exception:
            self.eng.close()
            raise

    def _add(self, clips):
        fo = np.concatenate([[0], np.cumsum([len(c[1]) for c in clips])]).astype(np.int64)
        self.eng.index_add_batch([c[0] for c in clips], fo, np.concatenate([c[1] for c in clips]).astype(np.int32),
                                 np.concatenate([c[2] for c in clips]).astype(np.int32))
        self.eng.index_set_scope([c[0] for c in clips], [c[3] for c in clips])

    def _late(self):
        self._add(self.late)
        self.eng.index_commit()
        for u in self.gone:
            self.eng.index_remove(u)
        self.eng.index_commit()

    def restore(self):
        """The late clips back in delta columns, if a search has merged them."""
        if self.name == "main" or self.eng.index_delta_stats()[1] == self.dsize:
            return
        assert self.eng.index_delta_stats()[1] == 0
        for c in self.late:
            if c[0] not in self.gone:
                self.eng.index_remove(c[0])
        self.eng.index_commit()
        self._late()
        assert self.eng.index_delta_stats()[1] == self.dsize

    def delta_clips(self):
        return self.eng.index_delta_stats()[1]


@pytest.fixture(scope="module")
def states(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    held = {}

    def get(name):
        if name not in held:
            held[name] = State(tfp_lib, name)
        return held[name]
    yield get
    for st in held.values():
        st.eng.close()


# form -> (its counters, the keys that make up "vote", the key of "general"); None: no form counter
_COUNTERS = {
    "plain": (lambda e: e.search_path_stats(), ("small", "vote_class", "vote_gemm"), "general"),
    "ranked": (lambda e: e.rank_stats(), ("vote_batches",), "general_batches"),
    "scoped": (lambda e: e.scope_stats(), ("vote_batches",), "general_batches"),
    "census": (lambda e: e.census_stats(), ("vote_batches",), "general_batches"),
    "sliding": (lambda e: e.slide_stats(), ("vote_batches",), "general_batches"),
    "neighbours": (lambda e: e.neighbour_stats(), ("vote_batches",), "general_batches"),
}
# the vote form of these serves any tolerance (the key bitsets are built at it); the others' the ones delta_tol_ok names
_VOTE_AT_ANY_TOL = ("plain", "ranked", "scoped", "census")


def _votes(form, coefs, tol, in_range):
    return coefs == 1 and in_range and (form in _VOTE_AT_ANY_TOL or T.delta_tol_ok(tol))


def _delta_stays(form, coefs, tol, in_range):
    if not in_range:
        return False
    if coefs == 1:
        return T.delta_tol_ok(tol)
    return form == "plain" and 0.0 <= tol <= T.ORDER_MAX_TOL


def _call(st, form, coefs, tol, in_range, fn):
    """fn() on the state's engine with the delta in place, the form that served it and the delta's fate asserted."""
    st.restore()
    # (inf, nan: k +- tol is not finite, the frame is switched off before its key is looked at: no key is out of range)
    in_range = in_range or not math.isfinite(tol)
    cnt = _COUNTERS.get(form)
    before = cnt[0](st.eng) if cnt else None
    out = fn()
    where = (st.name, form, coefs, tol, in_range)
    if cnt:
        now = cnt[0](st.eng)
        vote = sum(now[k] - before[k] for k in cnt[1])
        general = now[cnt[2]] - before[cnt[2]]
        assert (vote, general) == ((1, 0) if _votes(form, coefs, tol, in_range) else (0, 1)), (where, before, now)
    if st.name != "main":
        assert st.delta_clips() == (st.dsize if _delta_stays(form, coefs, tol, in_range) else 0), where
    return out


def _cases():
    return [(coefs, tol) for coefs in (1, 2) for tol in T.TOLS]


def _q(sel):
    """(frames, qoff, query indices) of the queries sel."""
    q1, q2, qoff, _ = T.queries()
    idx = list(sel)
    fr = [T.frames(q1[qoff[i]:qoff[i + 1]], q2[qoff[i]:qoff[i + 1]]) for i in idx]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])]).astype(np.int64)
    return (np.concatenate(fr) if off[-1] else np.zeros(1, R.FRAME_DTYPE)), off, idx


def _plain(res):
    return [[] if r is None else [(r["audio_uuid"], r["match_count"])] for r in res]


def test_the_split_is_what_it_says():
    """Every key of IN's frames lies in the vote range, OUT's frame at 600.0 does not; every query is in one."""
    q1, _, qoff, _ = T.queries()
    assert len(qoff) - 1 == NQ and sorted(IN + OUT) == list(range(NQ))
    keys = lambda sel: np.concatenate([np.trunc(np.where(np.isfinite(q1[qoff[i]:qoff[i + 1]]), q1[qoff[i]:qoff[i + 1]], 0.0))
                                       for i in sel])
    assert np.abs(keys(IN)).max() <= 30 and keys(OUT).max() == 600 >= T.KEY_RANGE / 2


@pytest.mark.parametrize("state", STATES)
def test_plain_ranked_scoped(states, oracle, tfp_lib, state):
    """search_batch, search_ranked_batch and search_scoped_batch (scope ANY and each scope); the first ranked
    row is the plain answer."""
    st = states(state)
    eng = st.eng
    with N.cached_boxes():
        for coefs, tol in _cases():
            ref_all = T.reference(oracle, coefs, tol, st.live)
            p = tfp_lib.params(coefs, tol)
            for sel in (IN, OUT):
                fr, qoff, idx = _q(sel)
                ref, inr, where = [ref_all[i] for i in idx], sel is IN, (state, coefs, tol, sel is IN)
                res, fcs = _call(st, "plain", coefs, tol, inr, lambda: eng.search_batch(fr, qoff, p))
                assert _plain(res) == [r[:1] for r in ref], where
                assert list(fcs) == list(np.diff(qoff)) and all(r is None or r["frame_count"] == n for r, n in zip(res, fcs))
                ranked = [R.pairs(r) for r in _call(st, "ranked", coefs, tol, inr, lambda: eng.search_ranked_batch(fr, qoff, p, K))]
                assert ranked == [r[:K] for r in ref], where
                assert [r[:1] for r in ranked] == _plain(res), where
                for x in (T.ANY, 0, 1, 2):
                    rows = _call(st, "scoped", coefs, tol, inr, lambda: eng.search_scoped_batch(fr, qoff, p, [x] * len(idx), K))
                    assert [R.pairs(r) for r in rows] == [T.in_scope(r, x)[:K] for r in ref], (where, x)


@pytest.mark.parametrize("state", STATES)
def test_census(states, oracle, tfp_lib, state):
    """census_batch against census_util's histogram of the same result sets, scope ANY and scope 1."""
    st = states(state)
    sp = T.spec()
    nbins = 41
    with N.cached_boxes():
        for coefs, tol in _cases():
            ref_all = T.reference(oracle, coefs, tol, st.live)
            p = tfp_lib.params(coefs, tol)
            for sel in (IN, OUT):
                fr, qoff, idx = _q(sel)
                for x in (T.ANY, 1):
                    hist = _call(st, "census", coefs, tol, sel is IN,
                                 lambda: st.eng.census_batch(fr, qoff, p, None if x == T.ANY else [x] * len(idx), nbins))
                    pop = sum(1 for c in st.live if x == T.ANY or sp["scope"][c] == x)
                    exp = np.stack([CU.dense(CU.sparse(T.in_scope(ref_all[i], x)), pop, nbins) for i in idx])
                    assert np.array_equal(hist, exp), (state, coefs, tol, sel is IN, x, np.nonzero((hist != exp).any(1))[0][:5])


_ALIGN = {}


def _align_ref(oracle, qi, uuid, coefs, tol):
    key = (qi, uuid, coefs, repr(tol))
    if key not in _ALIGN:
        sp = T.spec()
        q1, q2, qoff, _ = T.queries()
        cl = sp["clips"][sp["uuids"].index(uuid)]
        _ALIGN[key] = A.brute_force(oracle, cl["m1"], cl["m2"], q1[qoff[qi]:qoff[qi + 1]], q2[qoff[qi]:qoff[qi + 1]], coefs, tol)
    return _ALIGN[key]


@pytest.mark.parametrize("state", STATES)
def test_aligned_and_align_batch(states, oracle, tfp_lib, state):
    """search_aligned_batch: the ranked rows, each alignment against align_util.brute_force on the clip's rows
    in frame order; align_batch on the clip ids those rows name gives the same four fields."""
    st = states(state)
    with N.cached_boxes():
        for coefs, tol in _cases():
            ref_all = T.reference(oracle, coefs, tol, st.live)
            p = tfp_lib.params(coefs, tol)
            for sel in (IN, OUT):
                fr, qoff, idx = _q(sel)
                where = (state, coefs, tol, sel is IN)
                rows = _call(st, "aligned", coefs, tol, sel is IN, lambda: st.eng.search_aligned_batch(fr, qoff, p, K))
                assert [R.pairs(r) for r in rows] == [ref_all[i][:K] for i in idx], where
                for i, rs in zip(idx, rows):
                    for r in rs:
                        assert A.four(r) == _align_ref(oracle, i, r["audio_uuid"], coefs, tol), (where, i, r)
                ids = np.asarray([[r["clip_id"] for r in rs] + [-1] * (K - len(rs)) for rs in rows], np.int32)
                al = st.eng.align_batch(fr, qoff, p, ids.reshape(-1), K)
                for j, rs in enumerate(rows):
                    assert [A.four(a) for a in al[j][:len(rs)]] == [A.four(r) for r in rs], (where, j)
                    assert all(A.four(a) == (0, 0, 0, 0) for a in al[j][len(rs):])


@pytest.mark.parametrize("state", STATES)
def test_sliding_and_sliding_aligned(states, oracle, tfp_lib, state):
    """Window 8, hop 4 over the two 40-frame queries (9 windows each, every key in range): every window's rows
    against the brute force of the window cut out on the host, its alignments against align_util.brute_force on
    the window's frames, and both against the engine's own scoped and aligned searches of the windows as queries."""
    st = states(state)
    eng = st.eng
    sp = T.spec()
    q1, q2, qoff, _ = T.queries()
    assert qoff[1] - qoff[0] == 40 and qoff[2] - qoff[1] == 40
    window, hop = 8, 4
    nw = tfp_lib.sliding_windows(40, window, hop)
    assert nw == 9
    fr = T.frames(q1[:80], q2[:80])
    starts = [r * 40 + w * hop for r in range(2) for w in range(nw)]
    wfr = np.concatenate([fr[s:s + window] for s in starts])
    woff = np.arange(len(starts) + 1, dtype=np.int64) * window
    clip, m1, m2 = T.flat(st.live)
    with N.cached_boxes():
        for coefs, tol in _cases():
            p = tfp_lib.params(coefs, tol)
            where = (state, coefs, tol)
            exp = [R.brute_force(oracle, sp["uuids"], clip, m1, m2, q1[s:s + window], q2[s:s + window], coefs, tol, -1, -1,
                                 limit=K) for s in starts]
            got = _call(st, "sliding", coefs, tol, True, lambda: eng.search_sliding_batch(fr, [0, 40, 80], p, window, hop, K))
            assert [R.pairs(r) for r in got[0] + got[1]] == exp, where
            gal = _call(st, "sliding aligned", coefs, tol, True,
                        lambda: eng.search_sliding_aligned_batch(fr, [0, 40, 80], p, window, hop, K))
            flat_al = gal[0] + gal[1]
            assert [R.pairs(r) for r in flat_al] == exp, where
            for s, rs in zip(starts, flat_al):
                for r in rs[:2]:
                    cl = sp["clips"][sp["uuids"].index(r["audio_uuid"])]
                    assert A.four(r) == A.brute_force(oracle, cl["m1"], cl["m2"], q1[s:s + window], q2[s:s + window], coefs,
                                                      tol), (where, s, r)
            own = _call(st, "scoped", coefs, tol, True, lambda: eng.search_scoped_batch(wfr, woff, p, [T.ANY] * len(starts), K))
            assert [R.pairs(r) for r in own] == exp, where
            own_al = _call(st, "aligned", coefs, tol, True, lambda: eng.search_aligned_batch(wfr, woff, p, K))
            assert [[A.four(r) for r in rs] for rs in own_al] == [[A.four(r) for r in rs] for rs in flat_al], where


def _near_clips(live):
    """Four live clips without a row past the key range (a named clip's rows are its frames), NULL rows among them."""
    sp = T.spec()
    near = [c for c in live if "d" not in sp["clips"][c]["pop"]]
    pick = [c for c in near if "e" in sp["clips"][c]["pop"]][:2] + [c for c in near if "e" not in sp["clips"][c]["pop"]][:2]
    assert len(pick) == 4 and all(np.abs(sp["clips"][c]["m1"][sp["clips"][c]["m1"] != T.NULL]).max() < 40 * T.M for c in pick)
    return pick


def _catalog(st):
    sp = T.spec()
    cat = N.Catalog(sp["uuids"], [(c["m1"], c["m2"]) for c in sp["clips"]], [int(x) for x in sp["scope"]])
    for c in range(T.NCLIPS):
        cat.alive[c] = c in st.live
    return cat


@pytest.mark.parametrize("state", STATES)
def test_neighbours(states, oracle, tfp_lib, state):
    """index_neighbours against the brute force of test_gpu_neighbours.py (neighbour_util.check: rows, frame
    counts, every row's alignment), scope ANY and the clips' own scopes: four clips whose rows all lie in the
    key range (two with NULL rows) in one call, and clip 44, all rows past the key range, in a call of its own."""
    st = states(state)
    cat = _catalog(st)
    with N.cached_boxes():
        for coefs, tol in _cases():
            for names, inr in ((_near_clips(st.live), True), ([T.FAR[0]], False)):
                for scopes in (None, [cat.scope[c] for c in names]):
                    _call(st, "neighbours", coefs, tol, inr,
                          lambda: N.check(st.eng, oracle, tfp_lib, cat, names, coefs, tol, K, scopes, compose=False))


@pytest.mark.parametrize("state", STATES)
def test_the_widest_tolerances_agree(states, oracle, tfp_lib, state):
    """2 * kKeyRange, 1e12 (where fmt6_bound starts to saturate), 1e13 and 1e300: every row with a max1 lies in
    every box (the premise: tests/test_tolerance_oracle.py, and the references are equal here), so every form
    answers the same at all four. The neighbours' premise covers frames of the queries' keys: clips without a
    row past the key range are named (test_neighbours compares clip 44 with the brute force at each tolerance)."""
    st = states(state)
    eng = st.eng
    sp = T.spec()
    fr, qoff, idx = _q(range(NQ))
    names = [sp["uuids"][c] for c in _near_clips(st.live)]
    for coefs in (1, 2):
        assert all(T.reference(oracle, coefs, t, st.live) == T.reference(oracle, coefs, T.WIDE_TOLS[0], st.live) for t in T.WIDE_TOLS)
        seen = []
        for tol in T.WIDE_TOLS:
            p = tfp_lib.params(coefs, tol)
            st.restore()
            seen.append((_plain(eng.search_batch(fr, qoff, p)[0]),
                         [R.pairs(r) for r in eng.search_ranked_batch(fr, qoff, p, K)],
                         [R.pairs(r) for r in eng.search_scoped_batch(fr, qoff, p, [1] * len(idx), K)],
                         [[(r["audio_uuid"], r["match_count"]) + A.four(r) for r in rs] for rs in eng.search_aligned_batch(fr, qoff, p, K)],
                         eng.census_batch(fr, qoff, p, None, 41).tolist(),
                         [[R.pairs(w) for w in rec] for rec in eng.search_sliding_batch(fr[:80], [0, 40, 80], p, 8, 4, K)],
                         [[[(r["audio_uuid"], r["match_count"]) + A.four(r) for r in w] for w in rec]
                          for rec in eng.search_sliding_aligned_batch(fr[:80], [0, 40, 80], p, 8, 4, K)],
                         [(r["frame_count"], [(x["audio_uuid"], x["match_count"]) + A.four(x) for x in r["neighbours"]])
                          for r in eng.index_neighbours(names, p, K)]))
        for tol, s in zip(T.WIDE_TOLS[1:], seen[1:]):
            for form, (a, b) in enumerate(zip(seen[0], s)):
                assert a == b, (state, coefs, tol, form)


def test_rows_between_1440_and_2147_db(oracle, tfp_lib):
    """One more clip whose rows lie where the index's own stop (tolerance_util.farthest_clip: to the ends of int32,
    on and beside k +- 2048), in delta columns beside the 64: plain, ranked and census at every tolerance against the
    brute force. (Kept out of the shared index: with it the widest tolerances would not agree.)"""
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    sp = T.spec()
    fm1, fm2 = T.farthest_clip()
    uuids = sp["uuids"] + [T.FARTHEST_UUID]
    clip, m1, m2 = T.flat()
    clip, m1, m2 = np.concatenate([clip, np.full(len(fm1), T.NCLIPS)]), np.concatenate([m1, fm1]), np.concatenate([m2, fm2])
    q1, q2, qo, _ = T.queries()
    st = State(tfp_lib, "delta", extra=[(T.FARTHEST_UUID, fm1, fm2, 1)])
    try:
        changed = 0
        with N.cached_boxes():
            for coefs, tol in _cases():
                p = tfp_lib.params(coefs, tol)
                ref_all = [R.brute_force(oracle, uuids, clip, m1, m2, q1[a:b], q2[a:b], coefs, tol, -1, -1) for a, b in zip(qo[:-1], qo[1:])]
                changed += ref_all != T.reference(oracle, coefs, tol)
                for sel in (IN, OUT):
                    fr, qoff, idx = _q(sel)
                    ref, inr = [ref_all[i] for i in idx], sel is IN
                    res, _ = _call(st, "plain", coefs, tol, inr, lambda: st.eng.search_batch(fr, qoff, p))
                    assert _plain(res) == [r[:1] for r in ref], (coefs, tol, inr)
                    rows = _call(st, "ranked", coefs, tol, inr, lambda: st.eng.search_ranked_batch(fr, qoff, p, 32))
                    assert [R.pairs(r) for r in rows] == [r[:32] for r in ref], (coefs, tol, inr)
                    hist = _call(st, "census", coefs, tol, inr, lambda: st.eng.census_batch(fr, qoff, p, None, 41))
                    assert np.array_equal(hist, np.stack([CU.dense(CU.sparse(r), T.NCLIPS + 1, 41) for r in ref])), (coefs, tol, inr)
        assert changed >= 2 * 5  # (the clip is found from 2 * kKeyRange on at the least: it decides something)
    finally:
        st.eng.close()


def test_delta_in_place_at_8_and_merged_above(states, oracle, tfp_lib):
    """coefs = 1, every key in range, the two tolerances in direct succession on one delta: at 8.0 the dozen clips
    are still in delta columns after every form's call and at 8.000001 they have been merged (_call asserts both,
    and the form), and the results at both are the reference's."""
    st = states("delta")
    eng = st.eng
    fr, qoff, idx = _q(IN)
    q40, off40 = fr[:80], [0, 40, 80]
    q1, q2, _, _ = T.queries()
    sp = T.spec()
    cat = _catalog(st)
    names = _near_clips(st.live)
    clip, m1, m2 = T.flat(st.live)
    starts = [r * 40 + w * 4 for r in range(2) for w in range(9)]
    for tol in (T.DELTA_MAX_TOL, T.next_printed(T.DELTA_MAX_TOL)):
        p = tfp_lib.params(1, tol)
        ref = [T.reference(oracle, 1, tol, st.live)[i] for i in idx]
        win = [R.brute_force(oracle, sp["uuids"], clip, m1, m2, q1[s:s + 8], q2[s:s + 8], 1, tol, -1, -1, limit=K) for s in starts]
        res, _ = _call(st, "plain", 1, tol, True, lambda: eng.search_batch(fr, qoff, p))
        assert _plain(res) == [r[:1] for r in ref], tol
        rows = _call(st, "ranked", 1, tol, True, lambda: eng.search_ranked_batch(fr, qoff, p, K))
        assert [R.pairs(r) for r in rows] == [r[:K] for r in ref], tol
        rows = _call(st, "scoped", 1, tol, True, lambda: eng.search_scoped_batch(fr, qoff, p, [1] * len(idx), K))
        assert [R.pairs(r) for r in rows] == [T.in_scope(r, 1)[:K] for r in ref], tol
        rows = _call(st, "aligned", 1, tol, True, lambda: eng.search_aligned_batch(fr, qoff, p, K))
        assert [R.pairs(r) for r in rows] == [r[:K] for r in ref], tol
        for i, rs in zip(idx, rows):
            assert all(A.four(r) == _align_ref(oracle, i, r["audio_uuid"], 1, tol) for r in rs), (tol, i)
        hist = _call(st, "census", 1, tol, True, lambda: eng.census_batch(fr, qoff, p, None, 41))
        assert np.array_equal(hist, np.stack([CU.dense(CU.sparse(r), len(st.live), 41) for r in ref])), tol
        got = _call(st, "sliding", 1, tol, True, lambda: eng.search_sliding_batch(q40, off40, p, 8, 4, K))
        assert [R.pairs(r) for r in got[0] + got[1]] == win, tol
        got = _call(st, "sliding aligned", 1, tol, True, lambda: eng.search_sliding_aligned_batch(q40, off40, p, 8, 4, K))
        assert [R.pairs(r) for r in got[0] + got[1]] == win, tol
        _call(st, "neighbours", 1, tol, True, lambda: N.check(eng, oracle, tfp_lib, cat, names, 1, tol, K, compose=False))


def test_clip_order_cache_at_049_and_not_above(states, oracle, tfp_lib):
    """coefs = 2 (the general path) on a fresh engine: at kOrderMaxTol the clip-set cache is built from the clip
    order, at 0.490001 it is built and not from the order. With a delta and every key in range: at kOrderMaxTol
    the delta's own cache is swept beside the main one and the delta stays; at 0.490001 it is merged."""
    fr, qoff, idx = _q(range(NQ))
    lo, hi = T.ORDER_MAX_TOL, T.next_printed(T.ORDER_MAX_TOL)
    st = State(tfp_lib, "main")
    try:
        eng = st.eng
        st0 = eng.index_cache_stats()
        res, _ = eng.search_batch(fr, qoff, tfp_lib.params(2, lo))
        st1 = eng.index_cache_stats()
        assert _plain(res) == [r[:1] for r in T.reference(oracle, 2, lo)]
        assert (st1["builds"], st1["from_order"]) == (st0["builds"] + 1, st0["from_order"] + 1), (st0, st1)
        res, _ = eng.search_batch(fr, qoff, tfp_lib.params(2, hi))
        st2 = eng.index_cache_stats()
        assert _plain(res) == [r[:1] for r in T.reference(oracle, 2, hi)]
        assert (st2["builds"], st2["from_order"]) == (st1["builds"] + 1, st1["from_order"]), (st1, st2)
    finally:
        st.eng.close()
    fr, qoff, idx = _q(IN)
    st = states("delta")
    st.restore()
    st0 = st.eng.index_cache_stats()
    res, _ = _call(st, "plain", 2, lo, True, lambda: st.eng.search_batch(fr, qoff, tfp_lib.params(2, lo)))
    assert _plain(res) == [T.reference(oracle, 2, lo)[i][:1] for i in idx]
    assert st.eng.index_cache_stats()["delta_sweeps"] > st0["delta_sweeps"]  # (a redone speculative pass sweeps it twice)
    res, _ = _call(st, "plain", 2, hi, True, lambda: st.eng.search_batch(fr, qoff, tfp_lib.params(2, hi)))
    assert _plain(res) == [T.reference(oracle, 2, hi)[i][:1] for i in idx]


@pytest.mark.parametrize("state", STATES)
def test_live_calls(tfp_lib, state):
    """One live object per index state, three channels playing 8 kHz sources enrolled beside the tolerance index
    (in the delta and removed states their fingerprints sit in delta columns with the dozen, populations (b) and
    (c) among them): push and window after each of three ticks at tolerance_util.LIVE_TOLS, coefs 1 and 2, the
    last round switching tolerance between its ticks (8.0, 8.000001, 0.5: in place, merged, and searched merged).
    Expected: the scoped search of the call so far (live_util.prefix_rows) and of the kept frames of the window
    (live_window_util.definition_rows). After every push and window index_delta_stats: the delta is still in
    place for coefs = 1 at the tolerances delta_tol_ok names, merged otherwise."""
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    tick, nticks = 2048, 3
    pcm = tfp_lib.synth_pcm(0x701E, [0, 1, 2], 9000)
    nf = tfp_lib.frame_count(9000)
    src = ["ffff%04x-7070-4000-8000-00000000000%d" % (c, c) for c in range(3)]
    with tfp_lib.Engine(0) as fe:
        fp = fe.fingerprint_batch(np.concatenate(pcm), np.arange(4) * 9000)
    st = State(tfp_lib, state, extra=[(src[c], fp["m1"][c * nf:(c + 1) * nf], fp["m2"][c * nf:(c + 1) * nf], c) for c in range(3)])
    eng = st.eng
    try:
        assert state == "main" or st.dsize == len(T.DELTA) + 3 - len(st.gone)
        calls = np.stack([pcm[c][o:o + tick * nticks] for c, o in ((0, 256), (1, 333), (2, 1024))])
        scopes = [T.ANY, 1, 0]  # every clip, the source's own scope, another's
        lv = tfp_lib.Live(eng, 3, tick * nticks)
        found = 0
        rounds = [(coefs, (tol,) * nticks) for coefs in (1, 2) for tol in T.LIVE_TOLS]
        rounds.append((1, (T.DELTA_MAX_TOL, T.next_printed(T.DELTA_MAX_TOL), 0.5)))
        for coefs, tols in rounds:
            st.restore()
            lv.reset()
            hist = [np.zeros(0, np.int16)] * 3
            merged = False
            for t in range(nticks):
                where = (state, coefs, tols, t)
                p = tfp_lib.params(coefs, tols[t])
                merged = merged or not (coefs == 1 and T.delta_tol_ok(tols[t]))
                blk = calls[:, t * tick:(t + 1) * tick]
                hist = [np.concatenate([hist[c], blk[c]]) for c in range(3)]
                rows, fc = lv.push(blk, p, scopes, K)
                assert st.delta_clips() == (0 if merged else st.dsize), where
                assert fc == [tfp_lib.frame_count(len(h)) for h in hist], where
                wrows, wfc, wff = lv.window(p, scopes, K, 8)
                assert st.delta_clips() == (0 if merged else st.dsize), where
                assert rows == L.prefix_rows(eng, hist, p, scopes, K), where
                exp, efc, eff = LW.definition_rows(tfp_lib, eng, lv, p, scopes, K, 8)
                assert (wrows, wfc, wff) == (exp, efc, eff), where
                if not math.isfinite(tols[t]):
                    assert rows == [[], [], []] and wrows == [[], [], []]
                found += bool(rows[0])
        # A frame's own row lies in its box once the tolerance is 1 or more (|q1 - (int)q1| < 1, max2 exactly):
        # 1.0, 8.0, 8.000001 and kKeyRange for three ticks each and coefs, and two ticks of the switching round.
        assert found >= 2 * 4 * nticks + 2, found
        lv.close()
    finally:
        eng.close()
