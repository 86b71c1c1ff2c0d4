"""Shared by the aligned-search tests: the fixture and a numpy brute force of the alignment of a query
with one clip's rows (frame order), over the oracle's tfo_frame_box as ranked_util.brute_force:
hit(i, j) = frame i runs its SQL and row j lies in its box; hist[d] = the hits with j - i = d;
(aligned_count, offset, first_frame, last_frame) = (max hist, the smallest d attaining it, the least
and greatest i with hit(i, i + offset)), all 0 when nothing hits."""
import functools
import json
import math
import os

import numpy as np

import ranked_util as R

FIELDS = ("aligned_count", "offset", "first_frame", "last_frame")


@functools.lru_cache(maxsize=None)
def load_aligned():
    """{(scenario, query index): [(uuid, aligned_count, offset, first_frame, last_frame), ...rows 0..2]}."""
    with open(os.path.join(R.GOLDEN, "aligned_cases.json")) as f:
        doc = json.load(f)
    out = {}
    for name, qi, r, uuid, *four in doc["pairs"]:
        rows = out.setdefault((name, qi), [])
        assert len(rows) == r
        rows.append((uuid, *four))
    return out


def hit_matrix(oracle, m1, m2, q1, q2, coefs, tol, low, high):
    """bool [F, N]: hit(i, j)."""
    m1 = np.asarray(m1, np.int64)
    m2 = np.asarray(m2, np.int64)
    hits = np.zeros((len(q1), len(m1)), bool)
    if coefs < 1 or coefs > 2:  # fp_handler.c:247-250
        return hits
    tole = 0.001 if tol < 0 else tol  # fp_handler.c:252-256
    for i, (a, b) in enumerate(zip(q1, q2)):
        box = R.frame_box(oracle, -math.inf if a is None else a, -math.inf if b is None else b, coefs, tole, low, high)
        if box is None:
            continue
        L1, U1, has2, L2, U2 = box
        hit = (m1 != R.NULL) & (m1 >= L1) & (m1 <= U1)
        if has2:
            hit &= (m2 != R.NULL) & (m2 >= L2) & (m2 <= U2)
        hits[i] = hit
    return hits


def brute_force(oracle, m1, m2, q1, q2, coefs, tol, low=-1, high=-1, more=False):
    """(aligned_count, offset, first_frame, last_frame); with more, also the query frames with any hit
    and whether several diagonals attain the count."""
    hits = hit_matrix(oracle, m1, m2, q1, q2, coefs, tol, low, high)
    i, j = np.nonzero(hits)
    if not len(i):
        return ((0, 0, 0, 0), 0, False) if more else (0, 0, 0, 0)
    F = hits.shape[0]
    hist = np.bincount(j - i + F - 1)
    best = int(hist.max())
    off = int(np.argmax(hist)) - (F - 1)  # (argmax: the first, so the smallest, d)
    on = i[j - i == off]
    four = (best, off, int(on.min()), int(on.max()))
    return (four, len(np.unique(i)), int((hist == best).sum()) > 1) if more else four


def four(row):
    return tuple(row[f] for f in FIELDS)


def clip_rows(s, c):
    """Scenario s's clip c: its (m1, m2) rows in frame order."""
    sel = np.asarray(s["clip"], np.int64) == c
    return np.asarray(s["m1"], np.int64)[sel], np.asarray(s["m2"], np.int64)[sel]
