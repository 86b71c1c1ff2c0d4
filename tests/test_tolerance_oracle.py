"""The CPU oracle pinned at the tolerances where the engine changes its path (tolerance_util.TOLS), against
SQLite running the reference's own strings (oracle/sql_oracle.py, fp_handler.c:287-374), and the
tolerance index shown to decide something at every edge. No GPU, no engine: the code under test is
never used here.

Every tolerance of the list is served by SQLite, none by a fallback: "%f" of 1e300 is a 301-digit
literal SQLite reads as a real, and "%f" of inf / nan prints "inf" / "nan", which is no SQL literal:
the statement fails, db_ctx_exec logs it and the loop goes on (fp_handler.c:357-359), so no frame
inserts a row and the search is NOTFOUND with the frames counted."""
import math

import numpy as np
import pytest

import ranked_util as R
import tolerance_util as T


def _name(t):
    return repr(float(t))


# Neighbouring tolerances whose boxes print identically for every frame of the queries, per coefs; every other
# neighbouring pair changes some query's answer. Why these and no others:
#   0 / 4e-7 at coefs 1: max1 bounds are (int)max1 -+ tol, and "%f" of k -+ 4e-7 is k.000000 (at coefs 2 query
#       5's max2 values, a hair above their bases, print another bound at 4e-7)
#   2 * kKeyRange and above: every row with a max1 (and a max2) lies in every box
#   inf / nan: neither prints a literal
IDENTICAL = {1: {("0.0", "4e-07"), ("2048.0", "1000000000000.0"), ("1000000000000.0", "10000000000000.0"),
                 ("10000000000000.0", "1e+300"), ("inf", "nan")},
             2: {("2048.0", "1000000000000.0"), ("1000000000000.0", "10000000000000.0"),
                 ("10000000000000.0", "1e+300"), ("inf", "nan")}}


@pytest.fixture(scope="module")
def sql_cut():
    import sql_oracle
    sp = T.spec()
    db = sql_oracle.SqlFingerprintDB()
    db.insert_rows_bulk("ctx", [(sp["uuids"][c], sp["clips"][c]["m1"], sp["clips"][c]["m2"]) for c in T.SQL_CUT])
    return db


@pytest.mark.parametrize("coefs", [1, 2])
def test_oracle_equals_sqlite_at_every_tolerance(oracle, sql_cut, coefs):
    """oracle.search's (found, uuid, match_count, frame_count) == SQLite's, a dozen clips, every query."""
    sp = T.spec()
    q1, q2, qoff, _ = T.queries()
    clip, m1, m2 = T.flat(T.SQL_CUT)
    lit = lambda v: [None if not math.isfinite(x) else float(x) for x in v]  # an absent key (json_real(+-inf) is NULL)
    found_at = {}
    for tol in T.TOLS:
        for i, (a, b) in enumerate(zip(qoff[:-1], qoff[1:])):
            exp = sql_cut.search(lit(q1[a:b]), lit(q2[a:b]), coefs, tol, -1, -1)
            found, w, mc, fc = oracle.search(m1, m2, clip, sp["uuids"], q1[a:b], q2[a:b], coefs, tol, -1, -1)
            assert fc == b - a
            got = {"audio_uuid": sp["uuids"][w], "match_count": mc, "frame_count": fc} if found else None
            assert got == exp, (coefs, tol, i)
            found_at[_name(tol)] = found_at.get(_name(tol), 0) + found
    assert all(found_at[_name(t)] == 0 for t in T.NO_FRAME_TOLS), found_at
    assert all(found_at[_name(t)] > 0 for t in T.TOLS if math.isfinite(t)), found_at


@pytest.mark.parametrize("coefs", [1, 2])
def test_brute_force_equals_oracle_search_on_the_whole_index(oracle, coefs):
    """The result sets the GPU tests compare with (tolerance_util.reference: ranked_util.brute_force over the
    oracle's boxes) start with oracle.search's answer, at every tolerance, over all 64 clips."""
    sp = T.spec()
    q1, q2, qoff, _ = T.queries()
    clip, m1, m2 = T.flat()
    for tol in T.TOLS:
        ref = T.reference(oracle, coefs, tol)
        for i, (a, b) in enumerate(zip(qoff[:-1], qoff[1:])):
            found, w, mc, _ = oracle.search(m1, m2, clip, sp["uuids"], q1[a:b], q2[a:b], coefs, tol, -1, -1)
            assert ([(sp["uuids"][w], mc)] if found else []) == ref[i][:1], (coefs, tol, i)


@pytest.mark.parametrize("coefs", [1, 2])
def test_the_index_decides_at_every_edge(oracle, coefs):
    """Each neighbouring pair of tolerances changes some query's result set, or is one of IDENTICAL; more than
    half of the queries are found at every tolerance that runs a frame; a twin pair ties at the top somewhere."""
    sp = T.spec()
    nq = len(T.queries()[2]) - 1
    same = set()
    for lo, hi in zip(T.TOLS[:-1], T.TOLS[1:]):
        if T.reference(oracle, coefs, lo) == T.reference(oracle, coefs, hi):
            same.add((_name(lo), _name(hi)))
    assert same == IDENTICAL[coefs], (sorted(same - IDENTICAL[coefs]), sorted(IDENTICAL[coefs] - same))
    twins = {sp["uuids"][b]: sp["uuids"][a] for a, b in T.TWINS}
    tied = 0
    for tol in T.TOLS:
        ref = T.reference(oracle, coefs, tol)
        found = sum(1 for r in ref if r)
        print("coefs %d tolerance %r: %d of %d queries found" % (coefs, tol, found, nq))
        if math.isfinite(tol):
            assert 2 * found > nq, (coefs, tol, found)
        else:
            assert found == 0
        tied += sum(1 for r in ref if len(r) > 1 and twins.get(r[0][0]) == r[1][0] and r[0][1] == r[1][1])
    assert tied > 0


def test_the_widest_tolerances_hold_every_row(oracle):
    """The premise of the GPU test's equality of 2 * kKeyRange, 1e12, 1e13 and 1e300: at each of them every row
    with a max1 lies in every frame's max1 box, and every row with a max2 in every max2 box."""
    q1, q2, _, _ = T.queries()
    _, m1, m2 = T.flat()
    m1, m2 = m1[m1 != T.NULL], m2[m2 != T.NULL]
    for tol in T.WIDE_TOLS:
        for a, b in zip(q1, q2):
            L1, U1, has2, L2, U2 = R.frame_box(oracle, float(a), float(b), 2, tol, -1, -1)
            assert has2 and L1 <= m1.min() and m1.max() <= U1 and L2 <= m2.min() and m2.max() <= U2, (tol, a, b)
    # and one step down it no longer holds
    L1, U1 = R.frame_box(oracle, 30.2, 0.0, 1, T.KEY_RANGE, -1, -1)[:2]
    assert m1.min() < L1


def test_key_span_a_row_can_lie_in(oracle):
    """delta_bits looks for a delta row's keys within ceil(tol) + 1 of floor(max1): the index holds rows whose
    farthest key is exactly ceil(tol) away at 0.5, 1.0, 1.5 and 8.0 (a span of ceil(tol) - 1 misses them), and
    none lies farther at any tolerance delta_tol_ok admits. The + 1 is slack: max1 < floor(max1) + 1 and a
    printed bound never crosses an integer, so a key's box holds the row only within ceil(tol) of floor(max1);
    ceil(tol) + 1 -> ceil(tol) therefore changes no result, for any row."""
    _, m1, _ = T.flat()
    m1 = m1[m1 != T.NULL]
    kc = m1 // T.M  # (floor, as the kernel's)
    for tol in T.EDGE_TOLS:
        far = 0
        for k in range(-14, 42):
            L1, U1 = R.frame_box(oracle, float(k), 0.0, 1, tol, -1, -1)[:2]
            inside = (m1 >= L1) & (m1 <= U1)
            if inside.any():
                far = max(far, int(np.abs(kc[inside] - k).max()))
        assert far <= math.ceil(tol), (tol, far)
        if tol in (0.5, 1.0, 1.5, T.DELTA_MAX_TOL):
            assert far == math.ceil(tol), (tol, far)


def test_thresholds_are_the_sources(oracle):
    assert (T.ORDER_MAX_TOL, T.KEY_RANGE, T.DELTA_MAX_TOL) == (0.49, 1024, 8.0)  # what the issue's list was written for
    assert len(T.TOLS) == 22 and len({_name(t) for t in T.TOLS}) == 22
    assert np.all(np.diff([t for t in T.TOLS if t == t]) > 0)
