"""Catalog neighbours (tfp_index_neighbours, csrc/tfp_neighbour.hip): for each named clip the first k rows
of the reference's result query (fp_handler.c:367-374) for the clip's own stored rows, its own row
deleted, each with its alignment. The reference side is ranked_util.brute_force on the converted rows
with the self row deleted and align_util.brute_force; every case is also compared with the engine's
own composition (rows read back, scoped search at k + 1, align_batch). The form is asserted with
tfp_neighbour_stats."""
import ctypes as C

import numpy as np
import pytest

import neighbour_util as N
import ranked_util as R

pytestmark = pytest.mark.gpu

TFP_E_NOENT = -4
ANY = -1
M = 10**6
# Per scenario of tests/golden/match_cases.json: the named clips with at least one neighbour row, over coefs
# 1 and 2 and the fixture's distinct (tolerance, ignore low, ignore high) sets. Counted by
# ranked_util.brute_force alone (neighbour_util.ref_rows, no engine involved) on the fixture as committed;
# the sum is 11,010. A floor, so that a fixture or a parameter filter that silently empties the cases fails.
GOLDEN_CASES_WITH_ROWS = {"rand_00": 379, "rand_01": 376, "rand_02": 188, "rand_03": 303, "rand_04": 113, "rand_05": 518, "rand_06": 595,
                          "rand_07": 317, "rand_08": 52, "rand_09": 557, "rand_10": 52, "rand_11": 78, "rand_12": 187, "rand_13": 341,
                          "rand_14": 463, "rand_15": 147, "rand_16": 0, "rand_17": 197, "rand_18": 539, "rand_19": 357, "rand_20": 228,
                          "rand_21": 499, "rand_22": 302, "rand_23": 222, "tie_2000": 4000}


def _uuid(i):
    return "%08x-0000-4000-8000-%012x" % (i, i)


def _stats(eng):
    return eng.neighbour_stats()


def _form(eng, before, form):
    """One call since `before` was served by `form` ("vote" / "general")."""
    now = _stats(eng)
    other = "general" if form == "vote" else "vote"
    assert now[form + "_batches"] == before[form + "_batches"] + 1, (form, before, now)
    assert now[other + "_batches"] == before[other + "_batches"], (form, before, now)


def _param_sets(s):
    return sorted({(repr(q["tol"]), q["tol"], q["low"], q["high"]) for q in s["queries"] if q["coefs"] in (1, 2)})


def _golden_catalog(s):
    clip = np.asarray(s["clip"], np.int64)
    m1, m2 = np.asarray(s["m1"], np.int64), np.asarray(s["m2"], np.int64)
    return N.Catalog(s["uuids"], [(m1[clip == c], m2[clip == c]) for c in range(len(s["uuids"]))])


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES_WITH_ROWS))
def test_goldens_every_clip_named_k_1_3_32(engine, tfp_lib, oracle, name):
    """Every clip of the scenario named, coefs 1 and 2, every parameter set of the fixture. Rows against the
    brute force at k = 1, 3 and 32; every returned row's alignment against align_util.brute_force; at k = 1
    and 3 rows and alignments against the engine's own composition too."""
    s = R.load_cases()[0][name]
    cat = _golden_catalog(s)
    cat.enrol(engine)
    names = list(range(len(cat.uuids)))
    frames = [N.read_frames(engine, u) for u in cat.uuids]
    with_rows = 0
    with N.cached_boxes():
        for coefs in (1, 2):
            for _, tol, low, high in _param_sets(s):
                p = tfp_lib.params(coefs, tol, low, high)
                exp = [N.ref_rows(oracle, cat, c, coefs, tol, low, high) for c in names]
                with_rows += sum(1 for e in exp if e)
                al = [{} for _ in names]  # per named clip: neighbour uuid -> the brute force's alignment
                for k in (32, 3, 1):
                    res = engine.index_neighbours(cat.uuids, p, k)
                    assert N.got_rows(res) == [e[:k] for e in exp], (name, coefs, tol, low, high, k)
                    for c in names:
                        assert res[c]["frame_count"] == len(cat.m1[c])
                        for row in res[c]["neighbours"]:
                            u = row["audio_uuid"]
                            if u not in al[c]:
                                al[c][u] = N.ref_align(oracle, cat, c, u, coefs, tol, low, high)
                            assert N.A.four(row) == al[c][u], (name, coefs, tol, low, high, k, cat.uuids[c], u)
                    if k <= 31:
                        comp = N.composed_batch(engine, cat.uuids, frames, p, k, [ANY] * len(names))
                        for c in names:
                            rows = res[c]["neighbours"]
                            assert (R.pairs(rows), [N.A.four(r) for r in rows]) == comp[c], (name, coefs, tol, k, cat.uuids[c])
    print("golden cases with at least one neighbour row:", name, with_rows)
    assert with_rows >= GOLDEN_CASES_WITH_ROWS[name]


def _whole_clip(rng, n, keys):
    """n rows whose m1 are whole multiples of 10^6 (the clip's own row lies in every frame's box)."""
    return rng.choice(keys, n) * M, rng.integers(-40, 40, n) * M + rng.integers(0, M, n)


@pytest.mark.parametrize("own", [0, 1023, 1024])
def test_self_must_go_at_the_chunk_edge(engine, tfp_lib, oracle, own):
    """1,025 clips: the named clip matches itself on every frame, so it would be its own first row; its column
    is placed at 0, 1023, 1024 (the last of 1,025: the second block's only column)."""
    rng = np.random.default_rng(900 + own)
    n = 1025
    rows = [_whole_clip(rng, 3, np.arange(-5, 6)) for _ in range(n)]
    rows[own] = (np.array([1, 2, 3, 4]) * M, np.array([7, 8, 9, 10]) * M)
    rows[(own + 1) % n] = (np.array([1, 2, 3, 90]) * M, np.array([7, 8, 9, 10]) * M)  # three of its four frames
    cat = N.Catalog([_uuid(i) for i in range(n)], rows)  # (uuid order = column order)
    cat.enrol(engine)
    before = _stats(engine)
    res = N.check(engine, oracle, tfp_lib, cat, [own], 1, 0.001, 3, align_rows=1)
    _form(engine, before, "vote")
    assert cat.uuids[own] not in [u for u, _ in R.pairs(res[0]["neighbours"])]
    assert len(res[0]["neighbours"]) == 3
    # the composition sees the clip as its own first row, with a count of all four frames
    fr = R.frames_from_q(*cat.q(own))
    first = engine.search_scoped_batch(fr, [0, 4], tfp_lib.params(1, 0.001), [ANY], 1)[0][0]
    assert (first["audio_uuid"], first["match_count"]) == (cat.uuids[own], 4)
    N.check(engine, oracle, tfp_lib, cat, [own, (own + 1) % n], 2, 0.001, 32, compose=False, align_rows=1)


def test_self_as_row_k_plus_1_and_absent(engine, tfp_lib, oracle):
    """The named clip hits itself on one frame only, three others beat it: at k = 3 it would be row 4; and a
    clip whose values' fractions exceed the tolerance does not match itself at all (row k + 1 is dropped)."""
    a = (np.array([1 * M, 2 * M + 500000, 3 * M + 500000, 4 * M + 500000]), np.zeros(4, np.int64))
    others = [(np.array([1 * M, 2 * M, 3 * M, 4 * M]), np.zeros(4, np.int64)) for _ in range(4)]
    others[3] = (np.array([9 * M]), np.zeros(1, np.int64))
    cat = N.Catalog([_uuid(i) for i in range(5)], [a] + others)
    cat.enrol(engine)
    for coefs, tol, form in ((1, 0.3, "vote"), (2, 0.3, "general"), (1, 9.0, "general")):
        before = _stats(engine)
        N.check(engine, oracle, tfp_lib, cat, [0], coefs, tol, 3)
        _form(engine, before, form)
    frac = (np.array([1, 2, 3]) * M + 400000, np.zeros(3, np.int64))  # trunc +- 0.3 never holds x.4
    cat = N.Catalog([_uuid(i) for i in range(6)], [frac] + [(np.array([1, 2, 3]) * M + 100000 * (i % 3), np.zeros(3, np.int64))
                                                           for i in range(5)])
    cat.enrol(engine)
    for k in (1, 4, 5, 31, 32):
        res = N.check(engine, oracle, tfp_lib, cat, [0], 1, 0.3, k)
        assert len(res[0]["neighbours"]) == min(k, 5)


@pytest.mark.parametrize("own_key", [0, 2**31 - 1])
def test_self_with_a_tie_key_override(tfp_lib, oracle, own_key):
    rng = np.random.default_rng(77)
    n = 40
    rows = [_whole_clip(rng, 6, np.arange(-3, 4)) for _ in range(n)]
    cat = N.Catalog([_uuid(i) for i in range(n)], rows)
    with tfp_lib.Engine(0) as eng:
        cat.enrol(eng)
        keys = np.arange(1, n + 1, dtype=np.int32) * 5
        keys[17] = own_key
        eng.set_tiebreak(keys)
        key = {cat.uuids[i]: int(keys[i]) for i in range(n)}
        for k in (1, 3, 32):
            N.check(eng, oracle, tfp_lib, cat, [17, 3], 1, 0.001, k, key=key, align_rows=2)
        N.check(eng, oracle, tfp_lib, cat, [17], 2, 0.45, 4, key=key, align_rows=2)


@pytest.mark.parametrize("delta", ["1", "0"])
def test_index_delta(tfp_lib, oracle, monkeypatch, delta):
    """4,200 clips of 2 to 4 rows in one batch, then 3 added singly (with the delta: delta columns): a named
    clip in the delta with neighbours in main and the reverse, counts tied across main and delta."""
    monkeypatch.setenv("TFP_INDEX_DELTA", delta)
    rng = np.random.default_rng(4200)
    n = 4200
    rows = []
    for i in range(n):
        r = int(rng.integers(2, 5))
        rows.append((rng.integers(-400, 400, r) * M, rng.integers(-40, 40, r) * M))
    rows[100] = (np.array([450, 451, 452]) * M, np.array([1, 2, 3]) * M)
    rows[3000] = (np.array([450, 451, 499]) * M, np.array([1, 2, 3]) * M)
    cat = N.Catalog([_uuid(2 * i + 1) for i in range(n)], rows)
    with tfp_lib.Engine(0) as eng:
        cat.enrol(eng)
        eng.index_commit()
        eng.index_neighbours([cat.uuids[100]], tfp_lib.params(1, 0.001), 2)
        # sorted before, between and after the main columns' uuids; the first ties with clip 3000 (count 2)
        cat.add(eng, _uuid(0), np.array([450, 451, 480]) * M, np.array([1, 2, 3]) * M)
        cat.add(eng, _uuid(2 * 3000), np.array([450, 451, 452]) * M, np.array([1, 2, 9]) * M)
        cat.add(eng, _uuid(2 * n + 7), np.array([452, 460]) * M, np.array([3, 3]) * M)
        named = [100, 3000, n, n + 1, n + 2]
        for k in (1, 3, 32):
            before = _stats(eng)
            res = N.check(eng, oracle, tfp_lib, cat, named, 1, 0.001, k, compose=(k == 3))
            _form(eng, before, "vote")
        assert R.pairs(res[0]["neighbours"])[:3] == [(_uuid(2 * 3000), 3), (_uuid(2 * 3000 + 1), 2), (_uuid(0), 2)]
        if delta == "1":
            assert eng.index_delta_stats()[1] == 3  # the vote form never merged it
        N.check(eng, oracle, tfp_lib, cat, named, 2, 0.001, 3)


def _shape_catalog(rng):
    lens = [0, 1, 255, 256, 257, 300, 40, 40, 77, 12]
    rows = [(rng.integers(-6, 7, n) * M, rng.integers(-3, 4, n) * M) for n in lens]
    rows[6] = (np.full(40, R.NULL), np.full(40, R.NULL))              # all-NULL rows
    rows[7] = (rows[5][0][37:77].copy(), rows[5][1][37:77].copy())    # clip 5 from its row 37 on
    rows[8] = (rows[4][0][:77].copy(), rows[4][1][:77].copy())        # clip 4's first 77 rows
    rows[9] = (np.zeros(12, np.int64), np.zeros(12, np.int64))        # key 0
    return N.Catalog([_uuid(i) for i in range(len(lens))], rows)


def test_shapes(engine, tfp_lib, oracle):
    cat = _shape_catalog(np.random.default_rng(31))
    cat.enrol(engine)
    names = list(range(len(cat.uuids)))
    for coefs, tol, form in ((1, 0.001, "vote"), (1, 0.45, "vote"), (1, 9.0, "general"), (2, 0.001, "general"), (2, 0.45, "general")):
        for k in (1, 4, 32):
            before = _stats(engine)
            res = N.check(engine, oracle, tfp_lib, cat, names, coefs, tol, k, compose=(k == 4))
            _form(engine, before, form)
            assert _stats(engine)["frames_read"] == before["frames_read"] + sum(len(a) for a in cat.m1)
    res = N.check(engine, oracle, tfp_lib, cat, names, 1, 0.001, 32)
    assert res[0] == {"frame_count": 0, "neighbours": []}
    # all-NULL rows: the frames count; a NULL frame has key 0 (ast_json_real_get(NULL) = 0.0) and hits key 0's rows
    assert res[6]["frame_count"] == 40 and res[6]["neighbours"]
    assert all(np.any(cat.m1[cat.uuids.index(u)] == 0) for u, _ in R.pairs(res[6]["neighbours"]))
    # the copy from row 37: every frame of the copy hits on the diagonal 37 rows in
    r7 = {r["audio_uuid"]: r for r in res[7]["neighbours"]}[cat.uuids[5]]
    assert (r7["offset"], r7["first_frame"], r7["last_frame"]) == (37, 0, 39) and r7["aligned_count"] == 40
    r5 = {r["audio_uuid"]: r for r in res[5]["neighbours"]}[cat.uuids[7]]
    assert r5["offset"] == -37
    # an exact duplicate of a prefix: offset 0, aligned_count = the hitting frames
    r8 = {r["audio_uuid"]: r for r in res[8]["neighbours"]}[cat.uuids[4]]
    assert r8["offset"] == 0 and r8["aligned_count"] == r8["match_count"] == 77


def test_few_rows_removed_clips_twice_and_none(engine, tfp_lib, oracle):
    rng = np.random.default_rng(5)
    rows = [(np.arange(8) * M, np.zeros(8, np.int64)) for _ in range(3)] + [(np.array([100]) * M, np.zeros(1, np.int64))]
    cat = N.Catalog([_uuid(i) for i in range(4)], rows)
    cat.enrol(engine)
    p = tfp_lib.params(1, 0.001)
    res = N.check(engine, oracle, tfp_lib, cat, [0, 3, 0], 1, 0.001, 5)  # a uuid named twice; fewer rows than k
    assert res[0] == res[2] and len(res[0]["neighbours"]) == 2 and res[1]["neighbours"] == []
    # the tail past counts[i] is zeroed
    lib, k = tfp_lib.lib(), 5
    from tiresias_amd import _lib
    names = (C.c_char_p * 1)(cat.uuids[0].encode())
    out, al, cnt, fc = (_lib.Candidate * k)(), (_lib.Alignment * k)(), (C.c_int32 * 1)(), (C.c_int32 * 1)()
    C.memset(out, 0xAB, C.sizeof(out)), C.memset(al, 0xAB, C.sizeof(al))
    assert lib.tfp_index_neighbours(engine.handle, 1, names, C.byref(p), None, k, out, al, cnt, fc) == 0
    assert cnt[0] == 2 and fc[0] == 8
    assert bytes(out)[2 * C.sizeof(_lib.Candidate):] == bytes(3 * C.sizeof(_lib.Candidate))
    assert bytes(al)[2 * C.sizeof(_lib.Alignment):] == bytes(3 * C.sizeof(_lib.Alignment))
    # nclips = 0
    assert engine.index_neighbours([], p, 3) == []
    # a removed clip never appears, and naming it is TFP_E_NOENT with the outputs untouched
    engine.index_remove(cat.uuids[1])
    cat.alive[1] = False
    res = N.check(engine, oracle, tfp_lib, cat, [0], 1, 0.001, 5)
    assert R.pairs(res[0]["neighbours"]) == [(cat.uuids[2], 8)]
    N.check(engine, oracle, tfp_lib, cat, [0], 2, 0.001, 5)
    names = (C.c_char_p * 2)(cat.uuids[0].encode(), cat.uuids[1].encode())
    out2, cnt2 = (_lib.Candidate * (2 * k))(), (C.c_int32 * 2)(7, 7)
    C.memset(out2, 0xAB, C.sizeof(out2))
    before = _stats(engine)
    assert lib.tfp_index_neighbours(engine.handle, 2, names, C.byref(p), None, k, out2, None, cnt2, None) == TFP_E_NOENT
    assert list(cnt2) == [7, 7] and bytes(out2) == b"\xab" * C.sizeof(out2) and _stats(engine) == before
    with pytest.raises(tfp_lib.TfpError):
        engine.index_neighbours(["no-such-clip"], p, 1)


def test_scopes(engine, tfp_lib, oracle):
    rng = np.random.default_rng(8)
    n = 30
    rows = [_whole_clip(rng, 10, np.arange(-4, 5)) for _ in range(n)]
    cat = N.Catalog([_uuid(i) for i in range(n)], rows, [i % 3 for i in range(n)])
    cat.enrol(engine)
    names = [0, 1, 2, 4, 4]
    for coefs, tol in ((1, 0.001), (2, 0.45), (1, 9.0)):
        for scopes in ([0, 1, 2, 1, 1], [ANY] * 5, [1, 2, 0, 0, 2], [7, 7, 7, 7, ANY]):  # own, ANY, foreign, nobody's
            res = N.check(engine, oracle, tfp_lib, cat, names, coefs, tol, 4, scopes, align_rows=1)
            for i, sc in enumerate(scopes):
                if sc >= 0:
                    assert all(cat.scope[cat.uuids.index(u)] == sc for u, _ in R.pairs(res[i]["neighbours"]))
                if sc == 7:
                    assert res[i]["neighbours"] == []
    # a scope change between two calls
    a = N.check(engine, oracle, tfp_lib, cat, [0], 1, 0.001, 32, [1])
    moved = R.pairs(a[0]["neighbours"])[0][0]
    engine.index_set_scope([moved], [2])
    cat.scope[cat.uuids.index(moved)] = 2
    b = N.check(engine, oracle, tfp_lib, cat, [0], 1, 0.001, 32, [1])
    assert moved not in [u for u, _ in R.pairs(b[0]["neighbours"])]


def test_forms_out_of_range_key_and_no_alignment(engine, tfp_lib, oracle):
    rng = np.random.default_rng(12)
    n = 12
    rows = [_whole_clip(rng, 9, np.arange(-4, 5)) for _ in range(n)]
    rows[5] = (np.array([1, 2, 600, 600]) * M, np.zeros(4, np.int64))   # key 600: outside the vote range
    rows[6] = (np.array([1, 2, 600, 3]) * M, np.zeros(4, np.int64))
    cat = N.Catalog([_uuid(i) for i in range(n)], rows)
    cat.enrol(engine)
    before = _stats(engine)
    N.check(engine, oracle, tfp_lib, cat, [0, 1, 2], 1, 0.001, 3)
    _form(engine, before, "vote")
    before = _stats(engine)
    res = N.check(engine, oracle, tfp_lib, cat, [0, 5, 2], 1, 0.001, 3)  # redone on the general form
    _form(engine, before, "general")
    assert R.pairs(res[1]["neighbours"])[0] == (cat.uuids[6], 4)
    for k in (1, 32):
        before = _stats(engine)
        plain = N.check(engine, oracle, tfp_lib, cat, list(range(n)), 1, 0.45, k, aligned=False)
        assert _stats(engine)["pairs_aligned"] == before["pairs_aligned"]
        full = engine.index_neighbours(cat.uuids, tfp_lib.params(1, 0.45), k)
        assert N.got_rows(plain) == N.got_rows(full)
        assert _stats(engine)["pairs_aligned"] == before["pairs_aligned"] + sum(len(r["neighbours"]) for r in full)
