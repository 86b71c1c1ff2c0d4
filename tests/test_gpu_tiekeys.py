"""Tie-break keys at the edges of their range, through every search form, against the oracle.

A result is count << 32 | tie-break key, and once tfp_index_set_tiebreak / tfp_index_update_tiebreak
are used the caller chooses the keys (include/tiresias_fp.h: live clips' keys lie in [0, INT32_MAX],
distinct, ordered like the uuids). One synthetic index (integer rows, no audio) whose ties are decided
between the keys 0, 1, 2^24 - 1, 2^24, 2^24 + 1, 2^30, INT32_MAX - 1 and INT32_MAX goes through every
form; the expected rows come from the oracle and the brute-force count, which know uuids only
(count(*) DESC, audio_uuid DESC: src/fp_handler.c:367-374).

The index (_spec): 1,100 clips, clip number = uuid rank, added in shuffled order. Eight entities
e = 0..7 of 2 to 4 clips with the same rows under different uuids: a row in the box of every key in
[-300, 300] except key e - 4; a "weak" member also lacks key 4 (X). Every other clip lacks at least
two of the keys -4..3 and has a few rows elsewhere. A query for entity e has frames on every key of
-4..3 but e - 4 (so only entity e's members match every frame), with or without frames on X: with
X the full members beat the weak ones, without it the whole entity ties.

  (a) e = 0 with X: clip 1099 (key INT32_MAX) alone attains the count, the only clip of its pattern
  (b) e = 0 without X: it ties with clips 1098 (INT32_MAX - 1) and 300, same pattern
  (c) e = 1 with X: clip 0 (key 0) wins on its own (without X clip 1, key 1, wins the tie)
  (d) e = 2: the tie between columns 1023 and 1024, either side of the 1,024-clip vote chunk
      boundary, is decided between the keys 2^24 and 2^24 + 1
"""
import functools
import os

import numpy as np
import pytest

import ranked_util as R
import scoped_util as S

gpu = pytest.mark.gpu  # (every test but the construction check, which the non-GPU suite runs)

INT32_MAX = 2**31 - 1
NCLIPS = 1100
X = 4  # the key the weak members lack
# entity -> ([full members], [weak members]), clip numbers = uuid ranks
ENTITIES = {
    0: ([1099], [1098, 300]),
    1: ([0], [1]),
    2: ([1023, 1024], [1022]),
    3: ([1021, 1025, 700, 2], []),
    4: ([1060, 1059], [40]),
    5: ([1097, 511], [512]),
    6: ([255, 256, 1030], []),
    7: ([3], [5, 1090]),
}
EDGE_KEYS = (0, 1, 2**24 - 1, 2**24, 2**24 + 1, 2**30, INT32_MAX - 1, INT32_MAX)
ANY = -1  # TFP_SCOPE_ANY
ONLY_ZERO = 5  # the scope that holds clip 0 alone (the other clips: clip number % 3, as scoped_util)


def _tie_keys():
    """Clip number (uuid rank) -> override key: strictly increasing, through every edge key."""
    c = np.arange(NCLIPS, dtype=np.int64)
    k = np.where(c <= 1, c, 1 + (c - 1) * 16000)
    k = np.where(c >= 1022, 2**24 - 1 + (c - 1022), k)
    k = np.where(c > 1024, 2**24 + 1 + (c - 1024) * 1000000, k)
    k = np.where(c >= 1060, 2**30 + (c - 1060) * 2**24, k)
    k = np.where(c >= 1098, INT32_MAX - (1099 - c), k)
    assert (np.diff(k) > 0).all() and k[0] == 0 and k[-1] == INT32_MAX and set(EDGE_KEYS) <= set(k.tolist())
    return k.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _spec():
    rng = np.random.default_rng(0x71E)
    uuids = ["%08x-0000-4000-8000-%012x" % (c, c) for c in range(NCLIPS)]
    allkeys = np.arange(-300, 301)
    member = {}
    for e, (full, weak) in ENTITIES.items():
        keys = allkeys[allkeys != e - 4]
        m1 = (keys * 1000000 + rng.integers(-900, 901, len(keys))).astype(np.int32)
        m2 = (3000000 + rng.integers(-900, 901, len(keys))).astype(np.int32)
        for c in full:
            member[c] = (m1, m2)
        for c in weak:
            member[c] = (m1[keys != X], m2[keys != X])
    rows = []
    for c in range(NCLIPS):
        if c in member:
            rows.append(member[c])
            continue
        drop = set((rng.choice(8, 2, replace=False) - 4).tolist())
        keys = np.asarray([k for k in allkeys if k not in drop and rng.random() < (0.5 if -4 <= k <= 7 else 0.04)], np.int64)
        rows.append(((keys * 1000000 + rng.integers(-900, 901, len(keys))).astype(np.int32),
                     rng.integers(-5000000, 5000000, len(keys)).astype(np.int32)))
    scope = np.arange(NCLIPS) % S.CONTEXTS
    scope[0] = ONLY_ZERO
    return {"uuids": uuids, "rows": rows, "keys": _tie_keys(), "scope": scope.astype(np.int32),
            "order": rng.permutation(NCLIPS - 3)}  # (the top three uuids go last: the delta's clips)


def _flat(live):
    """(m1, m2, clip) of the live clips' rows."""
    sp = _spec()
    return (np.concatenate([sp["rows"][c][0] for c in live]), np.concatenate([sp["rows"][c][1] for c in live]),
            np.concatenate([np.full(len(sp["rows"][c][0]), c, np.int32) for c in live]))


@functools.lru_cache(maxsize=None)
def _queries(nq, extras, per_query, seed):
    """nq tie queries (entity i % 8, with X when (i // 8) % 2 == 0 so that 16 queries hold every case):
    1..3 frames on each of the entity's keys, and on per_query keys drawn from extras (keys outside
    -4..4: every member has them all). -> (q1, q2, qoff, entity[], with X[])."""
    rng = np.random.default_rng(seed)
    q1s, qoff, ent, wx = [], [0], [], []
    for i in range(nq):
        e, x = i % 8, (i // 8) % 2 == 0
        keys = [k for k in range(-4, 4) if k != e - 4] + ([X] if x else [])
        if extras:
            keys += rng.choice(extras, min(per_query, len(extras)), replace=False).tolist()
        cnt = rng.integers(1, 4 if len(keys) < 40 else 3, len(keys))
        k = np.repeat(np.asarray(keys, np.float64), cnt)[:120]
        f = rng.choice([0.2, 0.6], len(k))
        q1s.append(rng.permutation(np.where(k >= 0, k + f, k - f)))  # trunc(q1) == k
        qoff.append(qoff[-1] + len(k))
        ent.append(e), wx.append(x)
    q1 = np.concatenate(q1s)
    return q1, np.full(len(q1), 3.0), np.asarray(qoff, np.int64), tuple(ent), tuple(wx)


def _frames(q1, q2):
    fr = np.zeros(len(q1), R.FRAME_DTYPE)
    fr["q1"], fr["q2"] = q1, q2
    return fr


def _winner(e, x, live):
    full, weak = ENTITIES[e]
    cand = [c for c in full if c in live]
    if not x or not cand:
        cand += [c for c in weak if c in live]
    return max(cand)


_REF = {}


def _expect(oracle, qs, coefs, tol, live=None):
    """The oracle's (winner clip, count) per query over the live clips' rows (cached: computed once
    and shared), with the construction checked: every winner is the tie group's member the docstring
    names, with every frame matched, and (a) to (d) are all among the queries."""
    live = tuple(range(NCLIPS)) if live is None else live
    key = (id(qs), coefs, tol, live)
    if key not in _REF:
        q1, q2, qoff, ent, wx = qs
        m1, m2, clip = _flat(live)
        idx = oracle.SortedIndex(m1, m2, clip, np.arange(NCLIPS, dtype=np.int32))  # (tie key = uuid rank)
        w, mc = idx.search_batch(q1, q2, qoff, coefs, tol, -1, -1, nthreads=8)
        ls = set(live)
        want = np.asarray([_winner(e, x, ls) for e, x in zip(ent, wx)])
        in_range = np.asarray([np.all(np.abs(q1[a:b]) < 512) for a, b in zip(qoff[:-1], qoff[1:])])
        # (with clip 0 removed entity 1 has no full member left: its queries with X are anyone's)
        tie = np.asarray([0 in ls or e != 1 for e in ent])
        assert np.array_equal(w[tie], want[tie]), ("the construction: winners", np.nonzero(w != want)[0][:8])
        assert np.array_equal(mc[tie], (np.diff(qoff) - (~in_range).astype(np.int64))[tie]), "every frame matched"
        hit = {(e, x) for e, x in zip(ent, wx)}
        assert {(0, True), (0, False), (1, True), (2, True), (2, False)} <= hit  # (a) (b) (c) (d)
        _REF[key] = (w, mc)
    return _REF[key]


def _pairs_expected(oracle, qs, coefs, tol, live=None):
    sp = _spec()
    w, mc = _expect(oracle, qs, coefs, tol, live)
    return [(sp["uuids"][c], int(n)) for c, n in zip(w, mc)]


def _pairs(res):
    return [None if r is None else (r["audio_uuid"], r["match_count"]) for r in res]


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


def _enrol(eng, clips):
    sp = _spec()
    fo = np.concatenate([[0], np.cumsum([len(sp["rows"][c][0]) for c in clips])]).astype(np.int64)
    eng.index_add_batch([sp["uuids"][c] for c in clips], fo, np.concatenate([sp["rows"][c][0] for c in clips]),
                        np.concatenate([sp["rows"][c][1] for c in clips]))
    eng.index_set_scope([sp["uuids"][c] for c in clips], sp["scope"][list(clips)])


def _open(tfp_lib, env=None):
    """An engine with the whole index (shuffled uuid order, the top three uuids last) and its keys."""
    sp = _spec()
    eng = _engine_with(tfp_lib, env or {})
    try:
        ids = list(sp["order"]) + [NCLIPS - 3, NCLIPS - 2, NCLIPS - 1]
        _enrol(eng, ids)
        eng.set_tiebreak(sp["keys"][ids])
        eng.index_commit()
    except Exception:
        eng.close()
        raise
    return eng


# the query sets: 9 or 10 used keys (the small vote and the pattern-class vote), the used-key
# counts of test_vote_paths_vs_oracle for the three GEMM forms, and 12 keys
Q_FEW = lambda nq: _queries(nq, (), 0, 1)  # noqa: E731
Q_12 = lambda: _queries(40, (5, 6, 7), 3, 2)  # noqa: E731
Q_SPREAD = {4: lambda: _queries(40, (), 0, 3),  # keys -4..4
            40: lambda: _queries(40, tuple(k for k in range(-40, 41) if not -4 <= k <= 4), 50, 4),
            300: lambda: _queries(40, tuple(k for k in range(-300, 301) if not -4 <= k <= 4), 55, 5)}


def test_the_oracle_alone_satisfies_the_construction(oracle):
    """No engine: every query set's winners are the tie groups' members and (a) to (d) occur (_expect)."""
    for qs in [Q_FEW(16), Q_FEW(130), Q_12()] + [f() for f in Q_SPREAD.values()]:
        _expect(oracle, qs, 1, 0.001)
    for tol in (0.001, 0.45):
        _expect(oracle, Q_FEW(16), 2, tol)
    assert len(np.unique(np.trunc(Q_SPREAD[300]()[0]))) > 300 and len(np.unique(np.trunc(Q_SPREAD[40]()[0]))) > 60


@gpu
@pytest.mark.parametrize("nb", [1, 3, 8])
def test_small_vote(engine_keys, oracle, tfp_lib, nb):
    qs = Q_FEW(16)
    q1, q2, qoff = qs[:3]
    exp = _pairs_expected(oracle, qs, 1, 0.001)
    fr = _frames(q1, q2)
    for a in range(0, 16, nb):
        b = min(16, a + nb)
        res, fcs = engine_keys.search_batch(fr[qoff[a]:qoff[b]], qoff[a:b + 1] - qoff[a], tfp_lib.params(1, 0.001))
        assert _pairs(res) == exp[a:b], (nb, a)
        assert list(fcs) == list(np.diff(qoff[a:b + 1]))


@pytest.fixture(scope="module")
def engine_keys(tfp_lib):
    """The index under the default knobs, shared by the tests that change neither index nor knobs."""
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng = _open(tfp_lib)
    yield eng
    eng.close()


@gpu
@pytest.mark.parametrize("nq", [16, 130])
def test_pattern_class_vote(engine_keys, oracle, tfp_lib, nq):
    """At most 10 used keys under the default TFP_VOTE_CLASS_MAX: the class maxima carry key + 1,
    which for INT32_MAX needs all 32 bits (130 queries cross Qp = 128)."""
    qs = Q_FEW(nq)
    res, _ = engine_keys.search_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(1, 0.001))
    got, exp = _pairs(res), _pairs_expected(oracle, qs, 1, 0.001)
    bad = [(i, qs[3][i], qs[4][i], got[i], exp[i]) for i in range(nq) if got[i] != exp[i]]
    assert not bad, bad[:6]


@gpu
@pytest.mark.parametrize("class_max,which", [("-1", 4), ("-1", 40), ("-1", 300), ("10", 12)])
def test_vote_gemm(oracle, tfp_lib, class_max, which):
    """The GEMM with A in registers, through LDS and streamed: the fp32-packed accumulators carry
    the clip's position in its chunk, never a key (keys around 2^24 would not survive fp32)."""
    qs = Q_12() if which == 12 else Q_SPREAD[which]()
    eng = _open(tfp_lib, {"TFP_VOTE_CLASS_MAX": class_max})
    try:
        res, _ = eng.search_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(1, 0.001))
    finally:
        eng.close()
    assert _pairs(res) == _pairs_expected(oracle, qs, 1, 0.001), (class_max, which)


@gpu
@pytest.mark.parametrize("tol", [0.001, 0.45])
def test_sweep_by_groups(engine_keys, oracle, tfp_lib, tol):
    qs = Q_FEW(16)
    res, _ = engine_keys.search_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(2, tol))
    assert _pairs(res) == _pairs_expected(oracle, qs, 2, tol), tol


@functools.lru_cache(maxsize=None)
def _out_of_range_queries():
    """Q_FEW(16) with a 1000.0005 dB frame at the end of query 5: a key outside the vote range,
    which sends the coefs = 1 batch to the general path (test_search_small_out_of_range_key_falls_back)."""
    q1, q2, qoff, ent, wx = Q_FEW(16)
    at = int(qoff[6])
    q1 = np.insert(q1, at, 1000.0005)
    q2 = np.insert(q2, at, 3.0)
    qoff = qoff + (np.arange(17) >= 6)
    return q1, q2, qoff, ent, wx


@gpu
def test_cells_form_and_row_scan(oracle, tfp_lib):
    eng = _open(tfp_lib, {"TFP_WIDE_MIN_TOL": "1e9"})
    try:
        qs = _out_of_range_queries()
        res, _ = eng.search_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(1, 0.001))
        assert _pairs(res) == _pairs_expected(oracle, qs, 1, 0.001)
        for tol in (0.001, 0.45):
            qs = Q_FEW(16)
            res, _ = eng.search_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(2, tol))
            assert _pairs(res) == _pairs_expected(oracle, qs, 2, tol), tol
    finally:
        eng.close()


_BRUTE = {}


def _brute(oracle, qs, coefs, tol, keep=None, tag=None):
    """ranked_util.brute_force per query over the rows of the clips keep(clip number) (all: None)."""
    key = (id(qs), coefs, tol, tag)
    if key not in _BRUTE:
        sp = _spec()
        m1, m2, clip = _flat([c for c in range(NCLIPS) if keep is None or keep(c)])
        q1, q2, qoff = qs[:3]
        _BRUTE[key] = [R.brute_force(oracle, sp["uuids"], clip, m1, m2, q1[a:b], q2[a:b], coefs, tol, -1, -1)
                       for a, b in zip(qoff[:-1], qoff[1:])]
    return _BRUTE[key]


@gpu
@pytest.mark.parametrize("k", [1, 4, 6])
def test_ranked(engine_keys, oracle, tfp_lib, k):
    """K = 1, 4 and above the largest tie group (4 clips): a tie group's rows in descending uuid order."""
    sp = _spec()
    qs = Q_FEW(16)
    exp = _brute(oracle, qs, 1, 0.001)
    st0 = engine_keys.rank_stats()
    rows = engine_keys.search_ranked_batch(_frames(qs[0], qs[1]), qs[2], tfp_lib.params(1, 0.001), k)
    assert engine_keys.rank_stats()["vote_batches"] == st0["vote_batches"] + 1
    for i in range(16):
        assert R.pairs(rows[i]) == exp[i][:k], (k, i)
        full, weak = ENTITIES[qs[3][i]]
        top = sorted(full if qs[4][i] else full + weak, reverse=True)
        assert [u for u, _ in exp[i][:len(top)]] == [sp["uuids"][c] for c in top]  # the construction
        assert [r["audio_uuid"] for r in rows[i][:len(top)]] == [sp["uuids"][c] for c in top][:k]


def _in_scope(x):
    sp = _spec()
    return lambda c: sp["scope"][c] == x


@gpu
@pytest.mark.parametrize("k", [1, 4])
def test_scoped(engine_keys, oracle, tfp_lib, k):
    """Scope 1 holds the INT32_MAX clip; scope 0 excludes it (clip 1098, key INT32_MAX - 1, is the
    next member); ONLY_ZERO holds the key-0 clip alone. Expected: the brute-force count over the
    scope's rows (scoped_util.restrict: clip number % 3, less clip 0, which has a scope of its own)."""
    sp = _spec()
    qs = Q_FEW(16)
    s = {"uuids": sp["uuids"], "clip": _flat(range(NCLIPS))[2]}
    s["m1"], s["m2"] = _flat(range(NCLIPS))[:2]
    q1, q2, qoff = qs[:3]
    p = tfp_lib.params(1, 0.001)
    for x in (1, 0, ONLY_ZERO):
        if x == ONLY_ZERO:
            keep = s["clip"] == 0
            u, c, m1, m2 = s["uuids"], s["clip"][keep], s["m1"][keep], s["m2"][keep]
        else:
            u, c, m1, m2 = S.restrict(s, x)
            keep = c != 0
            c, m1, m2 = c[keep], m1[keep], m2[keep]
        exp = [R.brute_force(oracle, u, c, m1, m2, q1[a:b], q2[a:b], 1, 0.001, -1, -1, limit=k)
               for a, b in zip(qoff[:-1], qoff[1:])]
        rows = engine_keys.search_scoped_batch(_frames(q1, q2), qoff, p, [x] * 16, k)
        assert [R.pairs(r) for r in rows] == exp, (x, k)
        first = [e[0][0] if e else None for e in exp]
        for i in range(16):
            if qs[3][i] == 0 and x == 1:
                assert first[i] == sp["uuids"][1099]
            if qs[3][i] == 0 and x == 0 and not qs[4][i]:  # (without X the weak members match every frame)
                assert first[i] == sp["uuids"][1098]
            if x == ONLY_ZERO:
                assert first[i] == sp["uuids"][0]


@gpu
def test_sliding(engine_keys, oracle, tfp_lib):
    """A 120-frame recording, window 12, hop 3: 37 windows (two runs of at most 32), each window
    after a run's first updated from the one before. Expected: the brute-force count per window."""
    sp = _spec()
    q1, q2, qoff, ent, wx = Q_FEW(16)
    q1, q2 = q1[:120], q2[:120]
    window, hop, k = 12, 3, 4
    nw = tfp_lib.sliding_windows(120, window, hop)
    assert nw == 37 > tfp_lib._lib.TFP_SLIDE_RUN
    m1, m2, clip = _flat(range(NCLIPS))
    exp = [R.brute_force(oracle, sp["uuids"], clip, m1, m2, q1[w * hop:w * hop + window], q2[w * hop:w * hop + window], 1,
                         0.001, -1, -1, limit=k) for w in range(nw)]
    st0 = engine_keys.slide_stats()
    got = engine_keys.search_sliding_batch(_frames(q1, q2), [0, 120], tfp_lib.params(1, 0.001), window, hop, k)
    assert engine_keys.slide_stats()["vote_batches"] == st0["vote_batches"] + 1
    assert [R.pairs(r) for r in got[0]] == exp
    firsts = {e[0][0] for e in exp if e}
    assert sp["uuids"][1099] in firsts and len(firsts) > 3  # (windows inside query 0 are won by the INT32_MAX clip)


@gpu
def test_device_keys(engine_keys, oracle, tfp_lib):
    """tfp_search_q_device: the low half of each key maps back to the oracle's uuid through
    tfp_index_uuid_of_key, the high half is the oracle's count."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sp = _spec()
    assert engine_keys.uuid_of_key(0) == sp["uuids"][0] and engine_keys.uuid_of_key(INT32_MAX) == sp["uuids"][1099]
    for qs in (Q_FEW(3), Q_FEW(16), Q_12()):
        if len(qs[3]) < 16:
            w, mc = (np.asarray(a[:3]) for a in _expect(oracle, Q_FEW(16), 1, 0.001))  # (the same first 3 queries)
            assert np.array_equal(qs[0], Q_FEW(16)[0][:qs[2][-1]])
        else:
            w, mc = _expect(oracle, qs, 1, 0.001)
        d_q = torch.from_numpy(np.stack([qs[0], qs[1]], 1).copy()).cuda()
        keys = torch.zeros(len(w), dtype=torch.int64, device="cuda")
        engine_keys.search_q_device(d_q.data_ptr(), qs[2], tfp_lib.params(1, 0.001), keys.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        k = keys.cpu().numpy().view(np.uint64)
        assert np.array_equal((k >> np.uint64(32)).astype(np.int64), mc)
        low = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.array_equal(low, sp["keys"][w].astype(np.int64))
        assert [engine_keys.uuid_of_key(int(x)) for x in low] == [sp["uuids"][c] for c in w]
        assert {0, INT32_MAX} <= set(low.tolist()) or len(w) < 16


@gpu
@pytest.mark.parametrize("class_max", ["10", "-1"])
def test_index_delta(oracle, tfp_lib, class_max):
    """All but the top three uuids built and committed, then the three added with their keys by
    tfp_index_update_tiebreak: the INT32_MAX clip sits in a delta column, after the padding columns
    (key 0). Small vote, class vote / GEMM, ranked, scoped and the sweep (tolerance 0.001 and 0.45);
    all of them again without the key-0 clip."""
    sp = _spec()
    eng = _engine_with(tfp_lib, {"TFP_INDEX_DELTA": "1", "TFP_VOTE_CLASS_MAX": class_max})
    try:
        first = list(sp["order"])
        _enrol(eng, first)
        eng.set_tiebreak(sp["keys"][first])
        eng.index_commit()
        top = [NCLIPS - 3, NCLIPS - 2, NCLIPS - 1]
        _enrol(eng, top)
        eng.update_tiebreak(len(first), sp["keys"][top])
        eng.index_commit()
        assert eng.index_delta_stats()[1] == 3
        p = tfp_lib.params(1, 0.001)
        for live in (tuple(range(NCLIPS)), tuple(range(1, NCLIPS))):
            if live[0] == 1:
                eng.index_remove(sp["uuids"][0])
            ls = set(live)
            qs = Q_FEW(16)
            q1, q2, qoff = qs[:3]
            fr = _frames(q1, q2)
            exp = _pairs_expected(oracle, qs, 1, 0.001, live)
            for a in range(0, 16, 3):  # small vote
                b = min(16, a + 3)
                res, _ = eng.search_batch(fr[qoff[a]:qoff[b]], qoff[a:b + 1] - qoff[a], p)
                assert _pairs(res) == exp[a:b], (class_max, len(live), a)
            assert _pairs(eng.search_batch(fr, qoff, p)[0]) == exp, (class_max, len(live))  # class vote / GEMM
            big = Q_SPREAD[40]()
            assert _pairs(eng.search_batch(_frames(big[0], big[1]), big[2], p)[0]) == \
                _pairs_expected(oracle, big, 1, 0.001, live), (class_max, len(live))
            ranked = _brute(oracle, qs, 1, 0.001, keep=lambda c: c in ls, tag=len(live))
            rows = eng.search_ranked_batch(fr, qoff, p, 6)
            assert [R.pairs(r) for r in rows] == [e[:6] for e in ranked], (class_max, len(live))
            for x in (1, 0):
                sc = _brute(oracle, qs, 1, 0.001, keep=lambda c: c in ls and sp["scope"][c] == x, tag=(len(live), x))
                rows = eng.search_scoped_batch(fr, qoff, p, [x] * 16, 4)
                assert [R.pairs(r) for r in rows] == [e[:4] for e in sc], (class_max, len(live), x)
            # the sweep: with the delta it runs over the main clip-set cache and the delta's own
            # (tolerances up to 0.49), where the INT32_MAX clip's key is read from a delta column
            ds0 = eng.index_cache_stats()["delta_sweeps"]
            for tol in (0.001, 0.45):
                assert _pairs(eng.search_batch(fr, qoff, tfp_lib.params(2, tol))[0]) == \
                    _pairs_expected(oracle, qs, 2, tol, live), (class_max, len(live), tol)
            if live[0] == 0:  # (a removed clip of the sorted index merges the delta: the second pass has none)
                assert eng.index_delta_stats()[1] == 3  # served beside the main index, not merged
                assert eng.index_cache_stats()["delta_sweeps"] == ds0 + 2
    finally:
        eng.close()


# ---- the contract (include/tiresias_fp.h, tfp_index_set_tiebreak) -------------------------------

def _three(eng):
    for c in range(3):
        eng.index_add("00000000-0000-4000-8000-00000000000%d" % c, np.array([24000000 + c], np.int32),
                      np.array([0], np.int32))


@gpu
def test_negative_key_of_a_live_clip_fails_the_full_build(tfp_lib):
    eng = tfp_lib.Engine(0)
    try:
        _three(eng)
        eng.set_tiebreak([5, -1, 9])
        with pytest.raises(tfp_lib.TfpError, match="tie-break key -1 ") as ei:
            eng.index_commit()
        assert ei.value.code == -1  # TFP_E_ARG
        eng.set_tiebreak([5, 7, 9])
        eng.index_commit()
        assert eng.uuid_of_key(7).endswith("1")
    finally:
        eng.close()


@gpu
def test_negative_key_of_a_live_clip_fails_the_delta_update(tfp_lib):
    eng = _engine_with(tfp_lib, {"TFP_INDEX_DELTA": "1"})
    try:
        _three(eng)
        eng.set_tiebreak([5, 7, 9])
        eng.index_commit()
        eng.index_add("00000000-0000-4000-8000-000000000007", np.array([24000007], np.int32), np.array([0], np.int32))
        eng.update_tiebreak(3, [-1])
        upd0 = eng.index_delta_stats()[0]
        with pytest.raises(tfp_lib.TfpError, match="tie-break key -1 ") as ei:
            eng.index_commit()
        assert ei.value.code == -1
        eng.update_tiebreak(3, [INT32_MAX])
        eng.index_commit()
        assert eng.index_delta_stats() == (upd0 + 1, 1)  # (the delta path it was)
        assert eng.uuid_of_key(INT32_MAX).endswith("7")
    finally:
        eng.close()


@gpu
def test_key_of_a_removed_clip_is_ignored_and_int32_max_accepted(tfp_lib):
    eng = tfp_lib.Engine(0)
    try:
        _three(eng)
        eng.index_remove("00000000-0000-4000-8000-000000000001")
        eng.set_tiebreak([0, -1, INT32_MAX])
        eng.index_commit()
        assert eng.uuid_of_key(INT32_MAX).endswith("2") and eng.uuid_of_key(0).endswith("0")
        fr = _frames(np.array([24.2]), np.array([0.0]))
        r, _ = eng.search(fr, tfp_lib.params(1, 0.001))
        assert (r["audio_uuid"][-1], r["match_count"]) == ("2", 1)
    finally:
        eng.close()
