"""The occurrence fixture (tests/golden/occurrence_cases.json) checked by two independent routes and against
becoming an empty shell, and the new entry points' presence in the header and the ctypes binding. No GPU."""
import os
import subprocess
import sys

import align_util as A
import occurrence_util as O
import ranked_util as R
import slide_align_util as SA

NEW_SYMBOLS = ["tfp_trace_batch", "tfp_search_occurrences_batch", "tfp_search_occurrences_pcm_batch", "tfp_trace_stats",
               "tfp_group_search_occurrences_batch"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: the reference's predicate text run by SQLite per recording frame, byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_occurrences.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(os.path.join(R.GOLDEN, "occurrence_cases.json")) < 200_000


def test_occurrence_util_equals_every_trace_and_every_list(oracle):
    """Route 2: occurrence_util over align_util.hit_matrix (the oracle's frame_box) of the whole recording."""
    scen, _ = R.load_cases()
    cases, rows_of = O.load_occurrences(), SA.load_sliding_aligned()
    assert len(cases) == len(rows_of) > 48
    traces = lists = 0
    for (name, qi, window, hop, ctx, per), (name2, qi2, window2, hop2, ctx2, wins, _added) in zip(cases, rows_of):
        assert (name, qi, window, hop, ctx) == (name2, qi2, window2, hop2, ctx2)
        s, q = scen[name], scen[name]["queries"][qi]
        col = {u: c for c, u in enumerate(s["uuids"])}
        hits = {}

        def hit_matrix(uuid):
            if uuid not in hits:
                m1, m2 = A.clip_rows(s, col[uuid])
                hits[uuid] = A.hit_matrix(oracle, m1, m2, q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"])
            return hits[uuid]

        rows = [(0, r[0], w, r[3]) for w, win in enumerate(wins) for r in win[:SA.ROWS]]
        named = O.candidates_of_rows(rows, hop)
        assert len(per) == 2
        for max_gap, min_hits, tr, occ in per:
            assert [((0, u, st), n) for u, st, n, _ in tr] == sorted(named.items(), key=lambda kv: (col[kv[0][1]], kv[0][2]))
            for u, st, _n, t in tr:
                assert O.trace_of_hits(hit_matrix(u), st, max_gap) == t, (name, qi, window, hop, u, st, max_gap)
                traces += 1
            got = O.occurrences_of_rows(rows, hop, lambda _r, u, st: O.trace_of_hits(hit_matrix(u), st, max_gap), min_hits)
            assert got == occ, (name, qi, window, hop, max_gap, min_hits)
            lists += 1
    assert traces > 1000 and lists == 2 * len(cases)


def test_the_fixture_is_no_empty_shell():
    scen, _ = R.load_cases()
    cases = O.load_occurrences()
    joined = split = suppressed = low = 0
    for _name, _qi, _window, _hop, _ctx, per in cases:
        for _max_gap, min_hits, tr, occ in per:
            joined += sum(o["windows"] >= 2 for o in occ)                     # an occurrence named by two windows or more
            split += sum(t[2] >= 2 and t[3] < t[1] for _u, _s, _n, t in tr)   # several segments, the best short of all hits
            low += sum(t[3] < min_hits for _u, _s, _n, t in tr)               # dropped by min_hits
            suppressed += sum(t[3] >= min_hits for _u, _s, _n, t in tr) - len(occ)  # removed by suppression
    assert joined >= 1 and split >= 1 and suppressed >= 1 and low >= 1, (joined, split, suppressed, low)
    assert {scen[c[0]]["queries"][c[1]]["coefs"] for c in cases} == {1, 2}
    assert {c[4] < 0 for c in cases} == {True, False}  # unscoped and scoped
    assert {(g, m) for c in cases for g, m, _, _ in c[5]} == {(0, 1), (1, 2), (3, 3), (O.INT32_MAX, 2)}


def test_header_and_binding_have_the_new_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
