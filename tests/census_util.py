"""Shared by the census tests: the fixture (tests/golden/census_cases.json) and a brute-force census,
ranked_util.brute_force with no limit grouped by scope and histogrammed by count."""
import functools
import json
import os

import numpy as np

import ranked_util as R
import scoped_util as S

ANY = -1


@functools.lru_cache(maxsize=None)
def load_census():
    """{(scenario, query index): (census over all clips, of ctx0, of ctx1, of ctx2)}, census = ((count, clips), ...)."""
    with open(os.path.join(R.GOLDEN, "census_cases.json")) as f:
        doc = json.load(f)
    assert doc["contexts"] == ["ctx%d" % x for x in range(S.CONTEXTS)]
    return {(name, qi): tuple(tuple((c, n) for c, n in cen) for cen in per) for name, qi, per in doc["queries"]}


def sparse(pairs):
    """((count, clips), ...) by count descending from brute_force's [(uuid, count), ...]."""
    n = {}
    for _, c in pairs:
        n[c] = n.get(c, 0) + 1
    return tuple(sorted(n.items(), reverse=True))


def dense(census, population, nbins):
    """One row of nbins bins from ((count, clips), ...) with count >= 1; bin 0 closes to the population."""
    row = np.zeros(nbins, np.int32)
    for c, n in census:
        assert 1 <= c < nbins
        row[c] = n
    row[0] = population - int(row.sum())
    assert row[0] >= 0
    return row


def scenario_population(s, x):
    """Live clips of scope x (ANY: all) when clip c has scope c % 3 (scoped_util.enrol_scoped)."""
    n = len(s["uuids"])
    if x == ANY:
        return n
    return sum(1 for c in range(n) if c % S.CONTEXTS == x) if 0 <= x < S.CONTEXTS else 0


def brute_census(oracle, uuids, scope_of, clip, m1, m2, q1, q2, coefs, tol, low, high, scope, nbins):
    """The census row of one query: uuids are the live clips (row-less ones too), scope_of[uuid] their
    scopes, (clip, m1, m2) the rows by index into uuids."""
    rows = R.brute_force(oracle, uuids, clip, m1, m2, q1, q2, coefs, tol, low, high)
    mine = [(u, n) for u, n in rows if scope == ANY or scope_of[u] == scope]
    pop = sum(1 for u in uuids if scope == ANY or scope_of[u] == scope)
    return dense(sparse(mine), pop, nbins)
