"""Shared by the sliding-search tests: the per-window fixture (tests/golden/sliding_cases.json) and the
window arithmetic of include/tiresias_fp.h (window w = frames [w * hop, w * hop + window))."""
import functools
import json
import os

import ranked_util as R

RANKS = 4


def nwin(F, window, hop):
    return 0 if F < window else (F - window) // hop + 1


@functools.lru_cache(maxsize=None)
def load_sliding():
    """[(scenario name, query index, window, hop, context or -1, per window [(uuid, count), ...]), ...]."""
    with open(os.path.join(R.GOLDEN, "sliding_cases.json")) as f:
        doc = json.load(f)
    assert doc["ranks"] == RANKS and doc["contexts"] == ["ctx0", "ctx1", "ctx2"]
    scen, _ = R.load_cases()
    return [(name, qi, window, hop, ctx, [[(scen[name]["uuids"][c], n) for c, n in rows] for rows in wins])
            for name, qi, window, hop, ctx, wins in doc["cases"]]


def no_empty_shell(cases):
    """The generator's own assertions again: the rows reach below the winner, and the winner moves."""
    wins = [w for c in cases for w in c[5]]
    assert 3 * sum(len(w) >= 2 for w in wins) >= len(wins) > 0
    assert 5 * sum(len({w[0][0] if w else None for w in c[5]}) > 1 for c in cases) >= len(cases) > 0
