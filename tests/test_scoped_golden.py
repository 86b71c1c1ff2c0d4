"""The scoped-search fixture (tests/golden/scoped_cases.json) checked by three independent routes, and
the scoped entry points' presence in the header and the ctypes binding. No GPU."""
import os
import subprocess
import sys

import ranked_util as R
import scoped_util as S

NEW_SYMBOLS = ["tfp_index_set_scope", "tfp_index_scope", "tfp_search_scoped_batch", "tfp_search_scoped_pcm_batch",
               "tfp_scope_stats", "tfp_group_index_set_scope", "tfp_group_search_scoped_batch",
               "tfp_group_search_scoped_pcm_batch"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: peeling the reference's SQL per context (make_golden_scoped.py --check), byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_scoped.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_brute_force_over_the_contexts_clips_equals_peeled_rows(oracle):
    """Route 2: ranked_util.brute_force over the rows of the context's clips alone."""
    scen, ranked = R.load_cases()
    scoped = S.load_scoped()
    assert set(scoped) == set(ranked) and len(scoped) > 900  # every scenario and query of match_cases.json
    deep = differs = 0
    for (name, qi), per in scoped.items():
        s = scen[name]
        q = s["queries"][qi]
        for x in range(S.CONTEXTS):
            uuids, clip, m1, m2 = S.restrict(s, x)
            got = R.brute_force(oracle, uuids, clip, m1, m2, q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"],
                                limit=8)
            assert got == per[x], (name, qi, x)
            deep += len(per[x]) >= 2
            differs += bool(per[x]) and per[x][0] != ranked[(name, qi)][0]
    assert deep > 300     # the fixture does reach below each context's winner
    assert differs > 300  # and a context's winner is often not the global one


def test_contexts_merged_equal_the_ranked_fixture():
    """Route 3, the cross-pin: per query the three contexts' rows merged by (count descending, uuid
    descending) and cut to 8 equal ranked_cases.json's rows.

    Every query gets the full check (974 of 974), also where a context's list was cut at 8 rows: a row
    the cut dropped has 8 rows of its own context above it, so it lies at global row 9 or below and
    cannot be among ranked_cases.json's 8. No query needs the prefix-only check."""
    _, ranked = R.load_cases()
    scoped = S.load_scoped()
    full = 0
    for key, per in scoped.items():
        merged = sorted(((n, u) for rows in per for u, n in rows), reverse=True)[:8]
        assert [(u, n) for n, u in merged] == ranked[key], key
        assert len({u for rows in per for u, _ in rows}) == sum(len(rows) for rows in per)  # a clip is in one context
        full += 1
    assert full == len(ranked) > 900


def test_header_and_binding_have_the_scoped_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
    assert _lib.TFP_SCOPE_ANY == -1
