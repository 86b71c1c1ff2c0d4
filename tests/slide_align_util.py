"""Shared by the sliding-aligned-search tests: the per-window alignment fixture
(tests/golden/sliding_aligned_cases.json) and the alignments of every window of a recording with one
clip from a single hit matrix (align_util.hit_matrix over the whole recording): a window's hits are
the rows [w * hop, w * hop + window) of it, and its alignment is align_util.brute_force's arithmetic
on that slice."""
import functools
import json
import os

import numpy as np

import align_util as A
import ranked_util as R
import sliding_util as W

ROWS = 2
ZERO = (0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def load_sliding_aligned():
    """[(scenario name, query index, window, hop, context or -1, per window [(uuid, match_count,
    aligned_count, offset, first_frame, last_frame) for rows 0..1], added by the generator), ...]: the
    cases of sliding_cases.json in order, then the generator's own."""
    with open(os.path.join(R.GOLDEN, "sliding_aligned_cases.json")) as f:
        doc = json.load(f)
    assert doc["rows"] == ROWS
    sliding = W.load_sliding()
    assert len(doc["cases"]) == len(sliding)
    scen, _ = R.load_cases()
    out = []
    for (name, qi, window, hop, ctx, wins), (name2, qi2, window2, hop2, ctx2, fours) in zip(sliding, doc["cases"]):
        assert (name, qi, window, hop, ctx) == (name2, qi2, window2, hop2, ctx2) and len(wins) == len(fours)
        per = []
        for rows, fs in zip(wins, fours):
            assert len(fs) == min(len(rows), ROWS)
            per.append([(u, n, *f) for (u, n), f in zip(rows, fs)])
        out.append((name, qi, window, hop, ctx, per, False))
    for name, qi, window, hop, ctx, wins in doc["extra"]:
        per = [[(scen[name]["uuids"][c], n, *f) for c, n, *f in rows] for rows in wins]
        out.append((name, qi, window, hop, ctx, per, True))
    return out


def four_of_hits(h):
    """align_util.brute_force's result for the hit matrix h (bool [F, N]) of one query and one clip."""
    i, j = np.nonzero(h)
    if not len(i):
        return ZERO
    F = h.shape[0]
    hist = np.bincount(j - i + F - 1)
    best = int(hist.max())
    off = int(np.argmax(hist)) - (F - 1)  # (argmax: the first, so the smallest, d)
    on = i[j - i == off]
    return best, off, int(on.min()), int(on.max())


def window_fours(hits, window, hop):
    """Per window of the recording whose hit matrix with one clip is hits: its alignment."""
    return [four_of_hits(hits[w * hop:w * hop + window]) for w in range(W.nwin(hits.shape[0], window, hop))]
