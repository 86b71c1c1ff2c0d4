"""Aligned search (tfp_align_batch, tfp_search_aligned*, csrc/tfp_align.hip): per (query, candidate clip)
the diagonal row - frame with the most hits of the per-frame predicate (fp_handler.c:287-351), the
smallest such diagonal, and the first and last query frame on it, against the SQLite-derived fixture
tests/golden/aligned_cases.json and a numpy brute force (align_util.brute_force).

The kernel takes 256 diagonals per block (kAlignBand) and 256 query frames per LDS tile (kAlignTile),
64 of them per wave pass; the shapes below cross each of those edges."""
import ctypes as C

import numpy as np
import pytest

import align_util as A
import ranked_util as R

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_NOENT = -1, -4
BAND = TILE = 256
SEED = 0x7153A1
ZERO = (0, 0, 0, 0)


def _params(tfp_lib, q):
    return tfp_lib.params(q["coefs"], q["tol"], q["low"], q["high"])


def _ranked_part(rows):
    return [{k: r[k] for k in ("audio_uuid", "match_count", "clip_id")} for r in rows]


def _uuid(c):
    return "00000000-0000-4000-8000-%012d" % c


def test_goldens_k_1_and_3(engine, tfp_lib):
    scen, _ = R.load_cases()
    aligned = A.load_aligned()
    n = 0
    for name, s in scen.items():
        R.enrol(engine, s)
        by_p = {}
        for qi, q in enumerate(s["queries"]):
            if q["coefs"] in (1, 2):
                by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
        for qis in by_p.values():  # the queries of one parameter set as one batch
            p = _params(tfp_lib, s["queries"][qis[0]])
            frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis]
            qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
            for k in (1, 3):
                got = engine.search_aligned_batch(np.concatenate(frames), qoff, p, k)
                ranked = engine.search_ranked_batch(np.concatenate(frames), qoff, p, k)
                for i, rows, rrows in zip(qis, got, ranked):
                    exp = aligned.get((name, i), [])[:k]
                    assert _ranked_part(rows) == rrows, (name, i, k)  # cand and counts as the ranked search's
                    assert [(r["audio_uuid"],) + A.four(r) for r in rows] == exp, (name, i, k)
                    assert all(1 <= r["aligned_count"] <= r["match_count"] for r in rows)
                    n += k == 3
    engine.index_clear()
    assert n > 850


def test_entries_past_counts_are_zeroed(engine, tfp_lib):
    from tiresias_amd._lib import Alignment, Candidate
    scen, ranked = R.load_cases()
    # a query whose whole result set is 1..3 rows (the ranked fixture holds up to 8)
    name, qi = next(key for key, rows in ranked.items() if 1 <= len(rows) <= 3)
    s, nrows = scen[name], len(ranked[(name, qi)])
    R.enrol(engine, s)
    fr = R.frames_from_q(s["queries"][qi]["q1"], s["queries"][qi]["q2"])
    k = 8
    cand, align, counts = (Candidate * k)(), (Alignment * k)(), (C.c_int32 * 1)(-7)
    C.memset(align, 0xFF, C.sizeof(align))
    qoff = np.array([0, len(fr)], np.int64)
    p = _params(tfp_lib, s["queries"][qi])
    rc = tfp_lib.lib().tfp_search_aligned_batch(engine.handle, fr.ctypes.data, qoff.ctypes.data, 1, C.byref(p), k, cand,
                                                align, counts)
    assert rc == 0 and counts[0] == nrows and all(align[r].aligned_count >= 1 for r in range(nrows))
    assert bytes(align)[nrows * C.sizeof(Alignment):] == bytes((k - nrows) * C.sizeof(Alignment))
    engine.index_clear()


def test_align_batch_ids_and_arguments(engine, tfp_lib, oracle):
    from tiresias_amd._lib import Alignment
    scen, _ = R.load_cases()
    aligned = A.load_aligned()
    name = "rand_05"
    s = scen[name]
    R.enrol(engine, s)
    qi = max(range(len(s["queries"])), key=lambda i: len(aligned.get((name, i), [])))
    q = s["queries"][qi]
    exp = aligned[(name, qi)]
    assert len(exp) == 3
    fr, p = R.frames_from_q(q["q1"], q["q2"]), _params(tfp_lib, q)
    rows = engine.search_ranked(fr, p, 3)
    ids = [r["clip_id"] for r in rows]
    qoff = [0, len(fr)]
    # a ranked result's ids pass straight through, -1 gives a zeroed row, in any position
    got = engine.align_batch(fr, qoff, p, [ids[0], -1, ids[2], ids[1]], 4)[0]
    assert [A.four(g) for g in got] == [tuple(exp[0][1:]), ZERO, tuple(exp[2][1:]), tuple(exp[1][1:])]
    # a clip that was never a candidate aligns too (every clip against the brute force)
    for c, u in enumerate(s["uuids"]):
        m1, m2 = A.clip_rows(s, c)
        got = engine.align_batch(fr, qoff, p, [c], 1)[0][0]  # (enrol adds the clips in uuids order: clip id c)
        assert A.four(got) == A.brute_force(oracle, m1, m2, q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"]), u
    # no frames: zeros
    assert A.four(engine.align_batch(fr[:0], [0, 0], p, [ids[0]], 1)[0][0]) == ZERO
    for bad in (len(s["uuids"]), -2, 1 << 30):
        with pytest.raises(tfp_lib.TfpError) as ei:
            engine.align_batch(fr, qoff, p, [bad], 1)
        assert ei.value.code == TFP_E_NOENT
    engine.index_remove(rows[1]["audio_uuid"])
    with pytest.raises(tfp_lib.TfpError) as ei:
        engine.align_batch(fr, qoff, p, ids, 3)
    assert ei.value.code == TFP_E_NOENT
    assert [A.four(g) for g in engine.align_batch(fr, qoff, p, [ids[0], ids[2]], 2)[0]] == [tuple(exp[0][1:]), tuple(exp[2][1:])]
    out = (Alignment * 40)()
    idv = np.full(40, ids[0], np.int32)
    q2 = np.array(qoff, np.int64)
    for k, coefs in ((0, 1), (33, 1), (-1, 1), (2, 3), (2, 0)):
        pp = tfp_lib.params(coefs, 0.001)
        rc = tfp_lib.lib().tfp_align_batch(engine.handle, fr.ctypes.data, q2.ctypes.data, 1, C.byref(pp), idv.ctypes.data, k, out)
        assert rc == TFP_E_ARG, (k, coefs)
    engine.index_clear()


def _random_clip(rng, n, nulls=()):
    """n rows whose max1 / max2 lie in and just outside the boxes of keys 20..23 / 5..7."""
    m1 = rng.integers(20, 24, n) * 1_000_000 + rng.choice([-1500, -600, 0, 700, 1400], n)
    m2 = rng.integers(5, 8, n) * 1_000_000 + rng.choice([-470_000, -200_000, 0, 300_000, 460_000], n)
    m1, m2 = m1.astype(np.int64), m2.astype(np.int64)
    for j in nulls:
        m1[j] = R.NULL
    m2[rng.random(n) < 0.1] = R.NULL
    return m1, m2


def _random_query(rng, f):
    return list(rng.integers(19, 25, f) + 0.25), list(rng.integers(5, 8, f) + rng.choice([0.0, 0.3, 0.9], f))


def test_shapes_across_every_tile_edge(engine, tfp_lib, oracle):
    rng = np.random.default_rng(SEED)
    # N = 1, a short clip, N = 2 band + 1, N = 3 band - 1, first and last rows NULL, NULL rows only
    sizes = [1, 7, 40, 2 * BAND + 1, 3 * BAND - 1, 300, 100, 5]
    clips = [_random_clip(rng, n, nulls=(0, n - 1) if n == 300 else (range(n) if n == 5 else ())) for n in sizes]
    clips[0][0][0], clips[0][1][0] = 21_000_000, 6_000_000  # (the one-row clip lies inside key 21's boxes)
    engine.index_clear()
    for c, (m1, m2) in enumerate(clips):
        engine.index_add(_uuid(c), m1.astype(np.int32), m2.astype(np.int32))
    # F = 1, F > N, one wave pass +- 1, one frame tile +- 1, two tiles + 1
    lens = [1, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, 300, 2 * TILE + 1]
    queries = [_random_query(rng, f) for f in lens]
    frames = [R.frames_from_q(a, b) for a, b in queries]
    qoff = np.concatenate([[0], np.cumsum(lens)])
    k = len(clips)
    ids = np.tile(np.arange(k), len(lens))
    tied = negative = 0
    for coefs, tol in ((1, 0.001), (2, 0.001), (2, 0.45)):
        p = tfp_lib.params(coefs, tol)
        got = engine.align_batch(np.concatenate(frames), qoff, p, ids, k)
        for qi, (a, b) in enumerate(queries):
            for c, (m1, m2) in enumerate(clips):
                exp, _, tie = A.brute_force(oracle, m1, m2, a, b, coefs, tol, more=True)
                assert A.four(got[qi][c]) == exp, (coefs, tol, lens[qi], sizes[c])
                tied += tie
                negative += exp[1] < 0
        assert all(A.four(g[sizes.index(5)]) == ZERO for g in got)  # a clip of NULL rows never hits
        assert any(g[0]["aligned_count"] for g in got)  # N = 1 does
    assert tied > 50 and negative > 50
    # one query alone equals its row of the batch (single-pair launch)
    p = tfp_lib.params(2, 0.45)
    alone = engine.align_batch(frames[7], [0, lens[7]], p, [4], 1)[0][0]
    assert A.four(alone) == A.brute_force(oracle, *clips[4], *queries[7], 2, 0.45)
    engine.index_clear()


def test_ignore_filters_and_a_query_with_every_frame_ignored(engine, tfp_lib, oracle):
    rng = np.random.default_rng(SEED + 1)
    m1, m2 = _random_clip(rng, 400)
    engine.index_clear()
    engine.index_add(_uuid(0), m1.astype(np.int32), m2.astype(np.int32))
    a, b = _random_query(rng, 90)
    fr = R.frames_from_q(a, b)
    seen = 0
    # thresholds 10 log10(f): 150 -> 21.76 dB, 200 -> 23.01 dB; max2 filters: 4 -> 6.02 dB, 5 -> 6.99 dB
    for coefs, low, high in ((1, 150, -1), (1, -1, 200), (1, 150, 200), (2, 4, -1), (2, -1, 5), (2, 4, 200)):
        exp = A.brute_force(oracle, m1, m2, a, b, coefs, 0.45, low, high)
        plain = A.brute_force(oracle, m1, m2, a, b, coefs, 0.45)
        got = engine.align_batch(fr, [0, len(fr)], tfp_lib.params(coefs, 0.45, low, high), [0], 1)[0][0]
        assert A.four(got) == exp, (coefs, low, high)
        seen += exp != plain
    assert seen >= 4  # the filters do change the alignment
    # every frame below the low threshold (10 log10(1000) = 30 dB): no SQL runs
    p = tfp_lib.params(1, 0.45, 1000, -1)
    assert A.brute_force(oracle, m1, m2, a, b, 1, 0.45, 1000, -1) == ZERO
    assert A.four(engine.align_batch(fr, [0, len(fr)], p, [0], 1)[0][0]) == ZERO
    assert engine.search_aligned_batch(fr, [0, len(fr)], p, 3) == [[]]
    # tolerance < 0 selects the default
    assert A.four(engine.align_batch(fr, [0, len(fr)], tfp_lib.params(1, -1.0), [0], 1)[0][0]) == \
        A.brute_force(oracle, m1, m2, a, b, 1, -1.0)
    engine.index_clear()


@pytest.mark.parametrize("d0", [0, 1, 1023, 2040])
def test_known_offset_through_the_pcm_form(engine, tfp_lib, oracle, d0):
    """Samples [256 d0, 256 (d0 + 60)) of a 2,100-frame tfp_synth_pcm clip through the PCM form: the
    result equals the brute force on index_rows (checked first), and offset == d0 with aligned_count >= 59.

    The queried clip must have a time structure. Most tfp_synth_pcm clips are steady tones: clip 1 of this
    seed has max1 in [16.80, 16.90] dB in 1,115 of its frames from 900 on, so every frame of an excerpt has
    key 16, hit(i, j) depends on row j alone, and at tolerance 1.0 the diagonals 16, 942, 950, 951, ... all
    hold 60 hits (the definition then gives the smallest, 16, whatever d0 is). Clip 12 has a deep envelope
    and silent gaps: on the CPU oracle's fingerprints of its four excerpts the true diagonal is the one
    maximum of the histogram (60, 60, 59, 59 hits, no tie; so are clips 31, 33 and 39 of clips 0..47).
    That choice was made from the oracle's brute force, before any run of the kernel on it. Clips 1 and 31
    are enrolled beside it, the first as the steady-tone case."""
    nf = 2100
    pcm = tfp_lib.synth_pcm(SEED, [1, 12, 31], 256 * nf)
    fr = engine.fingerprint_batch(pcm.reshape(-1), np.arange(4) * 256 * nf)
    assert len(fr) == 3 * nf
    engine.index_clear()
    for c in range(3):
        engine.index_add(_uuid(c), fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    p = tfp_lib.params(1, 1.0)  # (a stored value always lies within 1 dB of its own truncation)
    q = pcm[1, 256 * d0:256 * (d0 + 60)]  # (row 1 of pcm: synthetic clip 12)
    got = engine.search_aligned_pcm_batch(q, [0, len(q)], p, 3)[0]
    f = engine.fingerprint(q)
    assert got == engine.search_aligned_batch(f, [0, 60], p, 3)[0]  # the frames form agrees
    rows = {r["audio_uuid"]: r for r in got}
    assert len(rows) == 3
    for c in range(3):
        m1, m2 = engine.index_rows(_uuid(c))
        assert A.four(rows[_uuid(c)]) == A.brute_force(oracle, m1, m2, list(f["q1"]), list(f["q2"]), 1, 1.0), c
    engine.index_clear()
    mine = rows[_uuid(1)]
    assert mine["aligned_count"] >= 59  # only the excerpt's first frame lacks its window history
    assert mine["offset"] == d0, mine


def test_no_commit_needed_and_the_live_delta(tfp_lib, oracle, monkeypatch):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    rng = np.random.default_rng(SEED + 2)
    clips = [_random_clip(rng, 120 + 10 * c) for c in range(5)]
    a, b = _random_query(rng, 50)
    fr, qoff = R.frames_from_q(a, b), [0, 50]
    with tfp_lib.Engine(0) as eng:
        for c in range(4):
            eng.index_add(_uuid(c), clips[c][0].astype(np.int32), clips[c][1].astype(np.int32))
        for coefs, tol in ((1, 0.001), (2, 0.45)):
            p = tfp_lib.params(coefs, tol)
            exp = [A.brute_force(oracle, m1, m2, a, b, coefs, tol) for m1, m2 in clips]
            # nothing committed, nothing searched: the staged rows are enough
            assert [A.four(g) for g in eng.align_batch(fr, qoff, p, [0, 1, 2, 3], 4)[0]] == exp[:4]
        eng.index_commit()
        eng.search(fr, tfp_lib.params(1, 0.001))
        cid = eng.index_add(_uuid(4), clips[4][0].astype(np.int32), clips[4][1].astype(np.int32))
        p = tfp_lib.params(1, 0.001)
        exp4 = A.brute_force(oracle, *clips[4], a, b, 1, 0.001)
        assert exp4[0] > 0
        before = eng.align_batch(fr, qoff, p, [cid], 1)[0][0]  # added, not committed
        eng.index_commit()
        assert eng.index_delta_stats()[1] == 1  # the clip is in the live delta
        after = eng.align_batch(fr, qoff, p, [cid], 1)[0][0]
        assert A.four(before) == A.four(after) == exp4
        rows = eng.search_aligned_batch(fr, qoff, p, 5)[0]  # the ranked search serves the delta beside the index
        assert eng.index_delta_stats()[1] == 1
        assert {r["audio_uuid"]: A.four(r) for r in rows}[_uuid(4)] == exp4


def test_staging_compaction_leaves_alignments_unchanged(tfp_lib, oracle):
    rng = np.random.default_rng(SEED + 3)
    big = [_random_clip(rng, 45_000) for _ in range(2)]  # removed: more than 2^16 dead rows forces a compaction
    small = [_random_clip(rng, 200 + 30 * c) for c in range(3)]
    a, b = _random_query(rng, 70)
    fr, qoff, p = R.frames_from_q(a, b), [0, 70], tfp_lib.params(2, 0.45)
    with tfp_lib.Engine(0) as eng:
        ids = []
        for c, (m1, m2) in enumerate([big[0], small[0], big[1], small[1], small[2]]):
            ids.append(eng.index_add(_uuid(c), m1.astype(np.int32), m2.astype(np.int32)))
        keep = [ids[1], ids[3], ids[4]]
        eng.index_commit()
        before = eng.align_batch(fr, qoff, p, keep, 3)[0]
        assert [A.four(g) for g in before] == [A.brute_force(oracle, m1, m2, a, b, 2, 0.45) for m1, m2 in small]
        full0 = eng.index_build_stats()[0]
        eng.index_remove(_uuid(0))
        eng.index_remove(_uuid(2))
        eng.index_commit()
        assert eng.index_build_stats()[0] > full0  # the full build that compacts the staging rows
        assert eng.align_batch(fr, qoff, p, keep, 3)[0] == before
        with pytest.raises(tfp_lib.TfpError):
            eng.align_batch(fr, qoff, p, [ids[0]], 1)


def test_align_stats_count_batches_and_pairs(tfp_lib):
    rng = np.random.default_rng(SEED + 4)
    a, b = _random_query(rng, 20)
    fr, p = R.frames_from_q(a, b), tfp_lib.params(1, 0.001)
    with tfp_lib.Engine(0) as eng:
        for c in range(3):
            m1, m2 = _random_clip(rng, 60)
            eng.index_add(_uuid(c), m1.astype(np.int32), m2.astype(np.int32))
        assert eng.align_stats() == {"batches": 0, "pairs": 0}
        eng.align_batch(np.concatenate([fr, fr]), [0, 20, 40], p, [0, 1, -1, 2, -1, -1], 3)
        assert eng.align_stats() == {"batches": 1, "pairs": 3}
        eng.align_batch(fr, [0, 20], p, [-1], 1)  # nothing to align: no launch
        assert eng.align_stats() == {"batches": 1, "pairs": 3}
        rows = eng.search_aligned_batch(fr, [0, 20], p, 2)[0]
        assert eng.align_stats() == {"batches": 2, "pairs": 3 + len(rows)} and rows


def test_group_of_three_equals_one_engine(tfp_lib):
    scen, _ = R.load_cases()
    aligned = A.load_aligned()
    g = tfp_lib.Group([0, 0, 0])
    try:
        n, shards = 0, set()
        for name in ("rand_05", "rand_09", "tie_2000"):
            s = scen[name]
            R.enrol(g, s)
            by_p = {}
            for qi, q in enumerate(s["queries"]):
                if q["coefs"] in (1, 2):
                    by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
            for qis in by_p.values():
                frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis]
                qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
                p = _params(tfp_lib, s["queries"][qis[0]])
                got = g.search_aligned_batch(np.concatenate(frames), qoff, p, 3)
                assert [_ranked_part(rows) for rows in got] == g.search_ranked_batch(np.concatenate(frames), qoff, p, 3)
                for i, rows in zip(qis, got):
                    assert [(r["audio_uuid"],) + A.four(r) for r in rows] == aligned.get((name, i), []), (name, i)
                    shards |= {r["clip_id"] for r in rows}
                    n += len(rows)
        assert len(shards) == 3  # the rows were aligned on every shard (tie_2000's three all lie on one)
        assert n > 100
    finally:
        g.close()
