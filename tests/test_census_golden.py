"""The census fixture (tests/golden/census_cases.json) checked by two independent routes, and against
the ranked and scoped fixtures it must contain. No GPU."""
import os
import subprocess
import sys

import census_util as U
import ranked_util as R
import scoped_util as S


def test_generator_check_reproduces_the_fixture():
    """Route 1: peeling the reference's SQL to exhaustion (make_golden_census.py --check), byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_census.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(os.path.join(R.GOLDEN, "census_cases.json")) < 1 << 20


def test_brute_force_histogrammed_equals_the_peeled_census(oracle):
    """Route 2: ranked_util.brute_force without a limit, over all clips and over each context's clips."""
    scen, ranked = R.load_cases()
    census = U.load_census()
    assert set(census) == set(ranked) and len(census) > 900  # every scenario and query of match_cases.json
    several = tied = 0
    for (name, qi), per in census.items():
        s = scen[name]
        q = s["queries"][qi]
        args = (q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"])
        assert U.sparse(R.brute_force(oracle, s["uuids"], s["clip"], s["m1"], s["m2"], *args)) == per[0], (name, qi)
        for x in range(S.CONTEXTS):
            assert U.sparse(R.brute_force(oracle, *S.restrict(s, x), *args)) == per[1 + x], (name, qi, x)
        several += len(per[0]) >= 2
        tied += any(n >= 2 for _, n in per[0])
    assert several > 200 and tied > 200  # the fixture has more than one bin, and bins of more than one clip
    assert census[("tie_2000", 0)][0] == ((census[("tie_2000", 0)][0][0][0], 2000),)  # 2,000 clips at one count


def test_census_contains_the_ranked_and_scoped_fixtures():
    """The cross-pin: read from the top, a census gives the counts of the first 8 rows of
    ranked_cases.json / scoped_cases.json, and the contexts' censuses add up to the one over all clips."""
    _, ranked = R.load_cases()
    scoped = S.load_scoped()
    census = U.load_census()

    def head(cen, k):
        return [c for c, n in cen for _ in range(n)][:k]

    for key, per in census.items():
        assert head(per[0], 8) == [n for _, n in ranked[key]], key
        total = {}
        for x in range(S.CONTEXTS):
            assert head(per[1 + x], 8) == [n for _, n in scoped[key][x]], (key, x)
            for c, n in per[1 + x]:
                total[c] = total.get(c, 0) + n
        assert tuple(sorted(total.items(), reverse=True)) == per[0], key
        assert all(c >= 1 and n >= 1 for cen in per for c, n in cen)
