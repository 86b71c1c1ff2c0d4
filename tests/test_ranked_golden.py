"""The ranked-search fixture (tests/golden/ranked_cases.json) checked by two independent routes, and
the ranked entry points' presence in the header and the ctypes binding. No GPU."""
import os
import subprocess
import sys

import ranked_util as R

NEW_SYMBOLS = ["tfp_search_ranked", "tfp_search_ranked_batch", "tfp_search_ranked_pcm_batch", "tfp_rank_stats",
               "tfp_group_search_ranked_batch", "tfp_group_search_ranked_pcm_batch"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: peeling the reference's SQL (make_golden_ranked.py --check), byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_ranked.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_brute_force_count_equals_peeled_rows(oracle):
    """Route 2: a numpy count over the scenario's rows with the oracle's frame boxes, sorted by
    (count descending, uuid descending), equals the peeled list of every stored query."""
    scen, ranked = R.load_cases()
    assert len(ranked) == sum(len(s["queries"]) for s in scen.values()) > 900
    deep = 0
    for (name, qi), rows in ranked.items():
        s = scen[name]
        q = s["queries"][qi]
        got = R.brute_force(oracle, s["uuids"], s["clip"], s["m1"], s["m2"], q["q1"], q["q2"], q["coefs"], q["tol"],
                            q["low"], q["high"], limit=8)
        assert got == rows, (name, qi)
        deep += len(rows) >= 2
    assert deep > 300  # the fixture does reach below the winner


def test_header_and_binding_have_the_ranked_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
