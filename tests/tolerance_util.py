"""Shared by the tolerance-edge tests: the tolerances at which a search changes its path, read out of
the sources, and one deterministic small index (integer rows, no audio) whose rows sit on, one
micro-unit inside and one outside the boxes those tolerances print (fp_handler.c:287-351: "%f" of
(int)max1 -+ tol, inclusive bounds).

The index (spec()): 64 clips of 5 to 40 rows, clip number = uuid rank, scope = clip number % 3, a few
clips twice under different uuids (TWINS: their counts tie, the greater uuid wins). A row is drawn for
a target (k, b), the key and the max2 base a query frame for it carries, from the populations

  (x) both values exactly on the target: what tolerance 0 can find
  (a) max1 within +-2000 micro-units of an integer key in [-3, 30]
  (b) max1 on k +- tol in micro-units, one inside, one outside, for every finite tolerance below 10
  (c) max1 on the half-integer k + 0.500000 (key k + 1 in the clip order, inside key k's inclusive
      box from 0.5 on) and on k +- 1.000000
  (d) max1 past the key range, 520 to 1440 dB either sign, among them rows on k + 600, k +- 1023.5
      and k +- 1024. Not beyond 1440: at 2 * kKeyRange every row has to lie in every frame's box
      (the frame at 600.0 reaches down to -1448), which is what makes the widest tolerances agree.
      The rows from 1440 dB to the ends of int32 are a clip of their own (farthest_clip()), enrolled
      only by the GPU test that compares them with the reference at every tolerance.
  (e) NULL max1, NULL max2, both

and max2 by the same recipe around b. No clip has more than 40 rows and no query more than 40 frames:
no count reaches a narrow counter's limit (40 * 40 < 2048) even when every row lies in every box.
"""
import functools
import math
import os
import re

import numpy as np

import ranked_util as R

M = 10**6
NULL = R.NULL
ANY = -1
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "asterisk-tiresias_amd", "csrc")


def _read(name, pattern):
    with open(os.path.join(_CSRC, name)) as f:
        m = re.search(pattern, f.read())
    if not m:
        raise AssertionError("%s no longer matches %r: tolerance_util reads its thresholds there" % (name, pattern))
    return float(m.group(1))


ORDER_MAX_TOL = _read("tfp_kernels.hpp", r"constexpr double kOrderMaxTol = ([0-9.]+);")
KEY_RANGE = _read("tfp_kernels.hpp", r"constexpr int32_t kKeyRange = (\d+);")
DELTA_MAX_TOL = _read("tfp_engine.cpp", r"bool delta_tol_ok\(double tol\) \{[^}]*tol <= ([0-9.]+);")


def next_printed(t):
    """The next tolerance above t that "%f" prints differently."""
    return float("%f" % (float("%f" % t) + 1e-6))


TOLS = (0.0, 4e-7, 5e-7, 6e-7, ORDER_MAX_TOL, next_printed(ORDER_MAX_TOL), 0.5, 0.999999, 1.0, 1.000001, 1.5,
        DELTA_MAX_TOL, next_printed(DELTA_MAX_TOL), 600.0, KEY_RANGE - 0.5, KEY_RANGE, 2 * KEY_RANGE, 1e12, 1e13, 1e300,
        math.inf, math.nan)
assert "%f" % TOLS[5] == "0.490001" and "%f" % TOLS[12] == "8.000001", TOLS
NO_FRAME_TOLS = tuple(t for t in TOLS if not math.isfinite(t))  # "%f" prints no SQL literal: no frame runs
WIDE_TOLS = (2 * KEY_RANGE, 1e12, 1e13, 1e300)  # every row with a max1 lies in every box
LIVE_TOLS = (0.0, 0.5, 1.0, DELTA_MAX_TOL, next_printed(DELTA_MAX_TOL), KEY_RANGE, math.inf)
EDGE_TOLS = tuple(t for t in TOLS if t < 10)  # population (b)


def same_tol(a, b):
    return a == b or (a != a and b != b)


NCLIPS = 64
TWINS = ((0, 1), (10, 11), (20, 23), (30, 31), (45, 58), (46, 47), (62, 63))  # (20, 23): one scope; the others two scopes
# Clips with no row near a key: at the tolerances that reach past the key range the other clips match every
# frame already, so only these decide there. 44: 40 rows of populations (d) and (e). 45 (and its twin 58, in the
# delta): 1026.000000 matches the frame of key 2 from kKeyRange on and not at kKeyRange - 0.5; 1053.500000 the
# frame of key 30 from kKeyRange - 0.5 on and not at 600; -1027.000001 the frame of key -3 above kKeyRange only.
FAR = (44, 45)
# A clip whose rows lie 18 keys apart: where the other clips match a frame through some other row once the
# tolerance is a few dB, this one (and its twin 47, in the delta) has one row per frame. 38.000001 matches the
# frame of key 30 from 8.000001 on and not at 8.0, -11.000000 the frame of key -3 from 8.0 on (on the bound),
# 19.999999 the frame of key 12 from 8.0 on (one inside).
SPARSE = 46
DELTA = (1, 5, 11, 17, 23, 29, 31, 40, 47, 52, 58, 63)  # added after the build: one of every twin pair, the top uuid
REMOVED = (31, 63)  # two clips of the delta, one a twin, one the top uuid: the delta stays beside the main index
# (removing a clip of the built index merges the delta at the next search, whatever the tolerance)


def delta_tol_ok(tol):
    """The tolerances at which a coefs = 1 vote form searches a live delta in place (tfp_engine.cpp)."""
    return math.isfinite(tol) and 0.0 <= tol <= DELTA_MAX_TOL
SQL_CUT = (0, 1, 10, 11, 20, 23, 30, 31, 44, 45, 62, 63)  # small enough for SQLite
NEIGHBOUR_CLIPS = (10, 44, 23, 7)  # 44: rows of population (d), 23: NULL rows (both asserted in spec())
EDGE_KEYS = (-3, -1, 0, 2, 7, 20)
BASES = (-2.0, 0.0, 3.0, 3.25, 5.0)


def _edge(rng):
    """A micro-unit offset on, one inside or one outside a finite tolerance's bound, either side."""
    t = int(round(float(rng.choice(EDGE_TOLS)) * M))
    return int(rng.choice([-1, 1])) * (t + int(rng.integers(-1, 2)))


def _row(rng, pops="xabcde"):
    """(m1, m2, k, b, population)."""
    k, b = int(rng.integers(-3, 31)), float(rng.choice(BASES))
    pop = rng.choice(list("xabcde"), p=[0.2, 0.2, 0.3, 0.12, 0.1, 0.08])
    if pop not in pops:
        pop = pops[0]
    off2 = 0 if rng.random() < 0.5 else int(rng.choice([_edge(rng), 500000, int(rng.integers(-2000, 2001))]))
    m1, m2 = k * M, int(round(b * M)) + off2
    if pop == "x":
        m2 = int(round(b * M))
    elif pop == "a":
        m1 += int(rng.integers(-2000, 2001))
    elif pop == "b":
        k = int(rng.choice(EDGE_KEYS))
        m1 = k * M + _edge(rng)
    elif pop == "c":
        m1 += int(rng.choice([500000, -500000, 1000000, -1000000]))
    elif pop == "d":
        k = int(rng.choice([-3, 2, 30]))
        far = [(k + 600) * M, (k + 1024) * M, (k - 1024) * M, (k + 1023) * M + 500000, (k - 1023) * M - 500000]
        m1 = int(rng.choice(far)) + int(rng.integers(-1, 2)) if rng.random() < 0.6 else \
            int(rng.choice([-1, 1])) * int(rng.integers(520 * M, 1440 * M))
        if rng.random() < 0.3:
            m2 += int(rng.choice([-600, 600])) * M
    else:
        which = int(rng.integers(3))
        m1, m2 = (NULL if which != 1 else m1), (NULL if which != 0 else m2)
    return m1, m2, k, b, pop


@functools.lru_cache(maxsize=None)
def spec():
    rng = np.random.default_rng(0x701E)
    lens = rng.integers(5, 41, NCLIPS)
    lens[[0, 44]] = 40
    lens[7] = 5
    clips = []
    for c in range(NCLIPS):
        rows = [_row(rng, "de" if c == FAR[0] else "xabcde") for _ in range(int(lens[c]))]
        if c == FAR[1]:  # one row per wide edge, each under a key of its own (see FAR)
            rows = [((2 + 1024) * M, 3 * M, 2, 3.0, "d"), (1053 * M + 500000, 3 * M, 30, 3.0, "d"),
                    (-1027 * M - 1, 3 * M, -3, 3.0, "d"), (NULL, 3 * M, 0, 3.0, "e"), (1440 * M, 3 * M, 7, 3.0, "d")]
        if c == SPARSE:
            rows = [(38 * M + 1, 0, 30, 0.0, "b"), (-11 * M, 0, -3, 0.0, "b"), (20 * M - 1, 0, 12, 0.0, "b"),
                    (NULL, 0, 0, 0.0, "e"), (38 * M + 1, NULL, 30, 0.0, "e")]
        clips.append({"m1": np.asarray([r[0] for r in rows], np.int64), "m2": np.asarray([r[1] for r in rows], np.int64),
                      "k": np.asarray([r[2] for r in rows], np.int64), "b": np.asarray([r[3] for r in rows]),
                      "pop": "".join(r[4] for r in rows)})
    for a, b in TWINS:
        clips[b] = clips[a]
    uuids = ["%08x-7070-4000-8000-%012x" % (c * 0x01010101 % 2**32, c) for c in range(NCLIPS)]
    assert uuids == sorted(uuids)
    sp = {"uuids": uuids, "clips": clips, "scope": np.arange(NCLIPS, dtype=np.int32) % 3,
          "order": [int(c) for c in rng.permutation(NCLIPS) if c not in DELTA]}
    # what the tests count on
    assert all(5 <= len(c["m1"]) <= 40 for c in clips) and set(clips[FAR[0]]["pop"]) <= set("de")
    dpop = "".join(clips[c]["pop"] for c in DELTA)
    assert "b" in dpop and "c" in dpop and "d" in dpop and "e" in dpop, dpop
    assert "d" in clips[NEIGHBOUR_CLIPS[1]]["pop"] and "e" in clips[NEIGHBOUR_CLIPS[2]]["pop"]
    far = np.concatenate([np.abs(c["m1"][c["m1"] != NULL]) for c in clips])
    assert far.max() <= 1440 * M and (far >= 520 * M).sum() > 60
    return sp


FARTHEST_UUID = "7f7f7f7f-7070-4000-8000-00000000007f"


def farthest_clip():
    """(m1, m2) of one more clip, enrolled by the test of the rows between 1440 and 2147 dB only (it is outside
    the premise of the widest tolerances): both signs, the ends of int32, rows on k +- 2048 for keys 2 and 30."""
    m1 = np.asarray([1441 * M, -1441 * M, 2147 * M, -2147 * M, 2**31 - 1, -(2**31) + 1, (2 + 2048) * M, (2 + 2048) * M + 1,
                     (30 - 2048) * M, (30 - 2048) * M - 1, 1800 * M + 500000, NULL], np.int64)
    return m1, np.full(len(m1), 3 * M, np.int64)


def flat(live=None):
    """(clip, m1, m2) of the live clips' rows (all: None), clip = index into spec()["uuids"]."""
    sp = spec()
    live = range(NCLIPS) if live is None else live
    return (np.concatenate([np.full(len(sp["clips"][c]["m1"]), c, np.int64) for c in live]),
            np.concatenate([sp["clips"][c]["m1"] for c in live]), np.concatenate([sp["clips"][c]["m2"] for c in live]))


def _q1_for(rng, k):
    """A max1 that truncates (toward zero) to key k, from either side of the half."""
    f = float(rng.choice([0.2, 0.7]))
    if k == 0:
        return float(rng.choice([0.2, 0.7, -0.3]))
    return k + f if k > 0 else k - f


@functools.lru_cache(maxsize=None)
def queries():
    """(q1, q2, qoff) of 24 queries: query i follows the targets of clip SOURCES[i]'s rows in row order (so that
    an alignment has a diagonal), 1 to 40 frames. Query 0 and 1: 40 frames (the sliding tests'); query 2: one
    frame; query 3: none; query 4: a non-finite q1 (key 0) and a frame at 600.0 (outside the vote's key range)
    among its frames; query 5: q2 a hair above its base, so that even 4e-7 moves a printed bound."""
    sp = spec()
    rng = np.random.default_rng(0x9E7)
    sources = [0, 44, 7, 3, 12, 9, 45, SPARSE] + [int(c) for c in rng.choice(NCLIPS, 16, replace=False)]
    q1s, q2s, qoff = [], [], [0]
    for i, c in enumerate(sources):
        cl = sp["clips"][c]
        n = {0: 40, 1: 40, 2: 1, 3: 0, 6: 5, 7: 5}.get(i, int(rng.integers(2, 41)))
        rows = [j for j in range(len(cl["m1"]))][:n]
        if i == 2:
            rows = [int(np.nonzero(np.asarray(list(cl["pop"])) == "x")[0][0])] if "x" in cl["pop"] else rows
        a = [_q1_for(rng, int(cl["k"][j])) for j in rows]
        b = [float(cl["b"][j]) for j in rows]
        if i == 4:
            a[0], a[-1] = math.inf, 600.0
        if i == 5:
            b = [v + 6e-7 for v in b]
        q1s += a
        q2s += b
        qoff.append(qoff[-1] + len(rows))
    q1, q2, qoff = np.asarray(q1s), np.asarray(q2s), np.asarray(qoff, np.int64)
    keys = np.trunc(np.where(np.isfinite(q1), q1, 0.0))
    assert keys.min() == -3 and keys.max() == 600 and np.any(q1 == -0.3) and np.diff(qoff).max() == 40
    assert {0, 1, 40} <= set(np.diff(qoff).tolist()) and len(qoff) == 25
    return q1, q2, qoff, tuple(sources)


def frames(q1, q2):
    fr = np.zeros(len(q1), R.FRAME_DTYPE)
    fr["q1"], fr["q2"] = q1, q2
    return fr


_REF = {}


def reference(oracle, coefs, tol, live=None):
    """Per query the whole result set [(uuid, count), ...] over the live clips' rows (ranked_util.brute_force),
    computed once per (coefs, tolerance, live clips) and shared."""
    key = (coefs, repr(tol), None if live is None else tuple(live))
    if key not in _REF:
        q1, q2, qoff, _ = queries()
        clip, m1, m2 = flat(live)
        _REF[key] = [R.brute_force(oracle, spec()["uuids"], clip, m1, m2, q1[a:b], q2[a:b], coefs, tol, -1, -1)
                     for a, b in zip(qoff[:-1], qoff[1:])]
    return _REF[key]


def in_scope(rows, scope):
    """A result set restricted to a scope: counts are per clip, so the scoped search's rows are these."""
    sp = spec()
    at = {u: c for c, u in enumerate(sp["uuids"])}
    return [r for r in rows if scope == ANY or sp["scope"][at[r[0]]] == scope]
