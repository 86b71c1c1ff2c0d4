"""Shared by the ranked-search tests: the fixtures and a brute-force count of the reference's result
set (fp_handler.c:287-374): per query frame the rows inside the frame's box, each clip once per frame
("group by audio_uuid" per insert), then the clips by (count descending, audio_uuid descending)."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NULL = -(2**31)
FRAME_DTYPE = np.dtype([("frame_idx", "<i4"), ("m1", "<i4"), ("m2", "<i4"), ("reserved", "<i4"),
                        ("q1", "<f8"), ("q2", "<f8")])


@functools.lru_cache(maxsize=None)
def load_cases():
    """(match_cases scenarios by name, ranked fixture as {(scenario, query index): [(uuid, count), ...]})."""
    with open(os.path.join(GOLDEN, "match_cases.json")) as f:
        scen = {s["name"]: s for s in json.load(f)["scenarios"]}
    with open(os.path.join(GOLDEN, "ranked_cases.json")) as f:
        doc = json.load(f)
    ranked = {(name, qi): [tuple(r) for r in rows] for name, qi, rows in doc["queries"]}
    return scen, ranked


def frames_from_q(q1, q2):
    fr = np.zeros(len(q1), FRAME_DTYPE)
    fr["q1"] = [-math.inf if v is None else v for v in q1]
    fr["q2"] = [-math.inf if v is None else v for v in q2]
    return fr


def frame_box(oracle, q1, q2, coefs, tole, low, high):
    """The oracle's tfo_frame_box: None (the frame runs no SQL) or (L1, U1, has2, L2, U2) in micro-units."""
    fn = oracle.lib().tfo_frame_box
    fn.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int] + [C.POINTER(C.c_int64)] * 2 + \
        [C.POINTER(C.c_int)] + [C.POINTER(C.c_int64)] * 2
    fn.restype = C.c_int
    L1, U1, L2, U2, has2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    if not fn(q1, q2, coefs, tole, low, high, C.byref(L1), C.byref(U1), C.byref(has2), C.byref(L2), C.byref(U2)):
        return None
    return L1.value, U1.value, bool(has2.value), L2.value, U2.value


def brute_force(oracle, uuids, clip, m1, m2, q1, q2, coefs, tol, low, high, limit=None):
    """[(uuid, count), ...] of every clip with a non-zero count, in the result set's order."""
    if coefs < 1 or coefs > 2:  # fp_handler.c:247-250
        return []
    tole = 0.001 if tol < 0 else tol  # fp_handler.c:252-256
    clip = np.asarray(clip, np.int64)
    m1 = np.asarray(m1, np.int64)
    m2 = np.asarray(m2, np.int64)
    counts = np.zeros(len(uuids), np.int64)
    for a, b in zip(q1, q2):
        box = frame_box(oracle, -math.inf if a is None else a, -math.inf if b is None else b, coefs, tole, low, high)
        if box is None:
            continue
        L1, U1, has2, L2, U2 = box
        hit = (m1 != NULL) & (m1 >= L1) & (m1 <= U1)
        if has2:
            hit &= (m2 != NULL) & (m2 >= L2) & (m2 <= U2)
        counts[np.unique(clip[hit])] += 1
    rows = sorted(((int(counts[c]), uuids[c]) for c in np.nonzero(counts)[0]), reverse=True)
    return [(u, n) for n, u in rows][:limit]


def enrol(engine, s):
    """The scenario's clips into an emptied engine (or group)."""
    engine.index_clear()
    clip = np.asarray(s["clip"], np.int64)
    m1 = np.asarray(s["m1"], np.int64).astype(np.int32)
    m2 = np.asarray(s["m2"], np.int64).astype(np.int32)
    if not s["uuids"]:
        return
    order = np.argsort(clip, kind="stable")
    fo = np.concatenate([[0], np.cumsum(np.bincount(clip, minlength=len(s["uuids"])))])
    engine.index_add_batch(s["uuids"], fo, m1[order], m2[order])


def pairs(rows):
    return [(r["audio_uuid"], r["match_count"]) for r in rows]
