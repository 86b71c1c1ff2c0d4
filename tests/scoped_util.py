"""Shared by the scoped-search tests: the per-context fixture (tests/golden/scoped_cases.json) and
the scenarios' context assignment (clip c in "ctx%d" % (c % 3), scope id c % 3)."""
import functools
import json
import os

import numpy as np

import ranked_util as R

CONTEXTS = 3
UNUSED_SCOPE = 7  # a scope no clip of the scenarios has


@functools.lru_cache(maxsize=None)
def load_scoped():
    """{(scenario, query index): ([(uuid, count), ...] of ctx0, of ctx1, of ctx2)}."""
    with open(os.path.join(R.GOLDEN, "scoped_cases.json")) as f:
        doc = json.load(f)
    assert doc["contexts"] == ["ctx%d" % x for x in range(CONTEXTS)] and doc["ranks"] == 8
    scen, _ = R.load_cases()  # the fixture names a clip by its index in the scenario's uuids
    return {(name, qi): tuple([(scen[name]["uuids"][c], n) for c, n in rows] for rows in per)
            for name, qi, per in doc["queries"]}


def restrict(s, x):
    """The scenario's (uuids, clip, m1, m2) with only the rows of context x's clips (clip ids kept)."""
    clip = np.asarray(s["clip"], np.int64)
    keep = clip % CONTEXTS == x
    return (s["uuids"], clip[keep], np.asarray(s["m1"], np.int64)[keep], np.asarray(s["m2"], np.int64)[keep])


def enrol_scoped(engine, s):
    """R.enrol, then clip c in scope c % 3."""
    R.enrol(engine, s)
    if s["uuids"]:
        engine.index_set_scope(s["uuids"], [c % CONTEXTS for c in range(len(s["uuids"]))])
