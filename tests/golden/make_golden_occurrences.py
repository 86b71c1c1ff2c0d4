"""Generate tests/golden/occurrence_cases.json — the diagonal traces and the occurrence lists of the
sliding-aligned fixture's rows.

For every case of sliding_aligned_cases.json (committed and extra: a query of match_cases.json taken as
the recording, a window, a hop, a context, rows 0 and 1 of every window with their alignment, so
k = 2), the candidates are the distinct (clip, s = w * hop - offset) over its rows, `windows` the rows
naming one. For the case's two (max_gap, min_hits) pairs (PAIRS below, chosen by the case's number),
each candidate's trace and the occurrence list.

The hits come from SQLite, not numpy: per recording frame x the reference's own predicate text
(fp_handler.c:287-351, make_golden_aligned.frame_predicate) runs as
    select audio_uuid, frame_idx from audio_fingerprint where <predicate>
against the scenario's table, so hit(x, j) of a clip = "(its uuid, j) is among frame x's rows". The
rest is plain Python from the definitions in include/tiresias_fp.h:
  trace: the frames x of [max(0, s), min(F, s + N)) with hit(x, x - s), cut into segments wherever
    x' - x - 1 > max_gap; (overlap, hits, segments, and the hits / first / last frame of the segment
    with the most hits, the earliest of equals); all but overlap 0 without a hit;
  occurrences: candidates with seg_hits < min_hits dropped; per clip the rest visited by seg_hits
    descending, windows descending, s ascending and kept unless [seg_first, seg_last] meets a kept
    one's; output by seg_first ascending, seg_hits descending, audio_uuid descending.

The file holds "cases": in the fixture's case order (committed, then extra), (scenario name, query
index, window, hop, context or -1, [[max_gap, min_hits, traces, occurrences] per pair]), with
traces = [[clip, s, windows, overlap, hits, segments, seg_hits, seg_first, seg_last], ...] by (clip, s)
and occurrences = [[clip, s, first_frame, last_frame, hits, diagonal_hits, overlap, windows], ...] in
output order, clip being the index of the audio_uuid in the scenario's "uuids".

Run:  python tests/golden/make_golden_occurrences.py            (writes the file)
      python tests/golden/make_golden_occurrences.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import json
import os
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, HERE)
from sql_oracle import SqlFingerprintDB  # noqa: E402

from make_golden_aligned import clip_rows, frame_predicate  # noqa: E402

INT32_MAX = 2 ** 31 - 1
PAIRS = [(0, 1), (1, 2), (3, 3), (INT32_MAX, 2)]  # case i takes PAIRS[i % 4] and PAIRS[(i + 2) % 4]
PATH = os.path.join(HERE, "occurrence_cases.json")


def frame_hits(db, q):
    """Per recording frame the set of (audio_uuid, frame_idx) its SQL returns (empty where it runs none)."""
    tole = q["tol"]
    if tole < 0:  # fp_handler.c:252-256
        tole = 0.001
    out = []
    for v1, v2 in zip(q["q1"], q["q2"]):
        pred = frame_predicate(v1, v2, q["coefs"], tole, q["low"], q["high"])
        rows = ()
        if pred is not None:
            try:
                rows = db.db.execute("select audio_uuid, frame_idx from audio_fingerprint where %s" % pred).fetchall()
            except sqlite3.Error:
                rows = ()  # the reference's insert fails the same way and its loop goes on (fp_handler.c:357-359)
        out.append(set(rows))
    return out


def trace(hits, uuid, N, s, max_gap):
    F = len(hits)
    lo, hi = max(0, s), min(F, s + N)
    overlap = max(0, hi - lo)
    xs = [x for x in range(lo, hi) if (uuid, x - s) in hits[x]]
    if not xs:
        return [overlap, 0, 0, 0, 0, 0]
    segs = [[xs[0]]]
    for a, b in zip(xs, xs[1:]):
        if b - a - 1 <= max_gap:
            segs[-1].append(b)
        else:
            segs.append([b])
    best = max(segs, key=lambda g: (len(g), -g[0]))
    return [overlap, len(xs), len(segs), len(best), best[0], best[-1]]


def occurrences(cands, uuids, min_hits):
    """cands = [[clip, s, windows, overlap, hits, segments, seg_hits, seg_first, seg_last]]: (the output list,
    candidates dropped by min_hits, candidates removed by suppression)."""
    kept, low, sup = [], 0, 0
    for clip in sorted({c[0] for c in cands}):
        mine = []
        for c in sorted((c for c in cands if c[0] == clip), key=lambda c: (-c[6], -c[2], c[1])):
            if c[6] < min_hits:
                low += 1
            elif any(c[7] <= k[8] and k[7] <= c[8] for k in mine):
                sup += 1
            else:
                mine.append(c)
        kept += mine
    # audio_uuid descending among equals: two sorts, the last one stable
    kept.sort(key=lambda c: uuids[c[0]], reverse=True)
    kept.sort(key=lambda c: (c[7], -c[6]))
    return [[c[0], c[1], c[7], c[8], c[6], c[4], c[3], c[2]] for c in kept], low, sup


def load_cases():
    """[(name, query index, window, hop, context, per window [(clip, offset) for rows 0..1 with a hit])]."""
    with open(os.path.join(HERE, "sliding_cases.json")) as f:
        sliding = json.load(f)["cases"]
    with open(os.path.join(HERE, "sliding_aligned_cases.json")) as f:
        doc = json.load(f)
    out = []
    for (name, qi, window, hop, ctx, wins), (_, _, _, _, _, fours) in zip(sliding, doc["cases"]):
        out.append((name, qi, window, hop, ctx, [[(c, f[1]) for (c, _n), f in zip(rows, fs)] for rows, fs in zip(wins, fours)]))
    for name, qi, window, hop, ctx, wins in doc["extra"]:
        out.append((name, qi, window, hop, ctx, [[(r[0], r[3]) for r in rows] for rows in wins]))
    return out


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        scen = {s["name"]: s for s in json.load(f)["scenarios"]}
    cases, out, dbs, hits_of = load_cases(), [], {}, {}
    seen = dict(joined=0, split=0, suppressed=0, low=0, occ=0)
    for i, (name, qi, window, hop, ctx, wins) in enumerate(cases):
        s = scen[name]
        if name not in dbs:
            dbs = {name: SqlFingerprintDB()}
            hits_of = {}
            for c, (m1s, m2s) in enumerate(clip_rows(s)):
                dbs[name].insert_rows("ctx%d" % (c % 3), s["uuids"][c], m1s, m2s)
        if qi not in hits_of:
            hits_of[qi] = frame_hits(dbs[name], s["queries"][qi])
        hits = hits_of[qi]
        nrows = [s["clip"].count(c) for c in range(len(s["uuids"]))]
        named = {}
        for w, rows in enumerate(wins):
            for clip, offset in rows:
                named[(clip, w * hop - offset)] = named.get((clip, w * hop - offset), 0) + 1
        per = []
        for max_gap, min_hits in (PAIRS[i % 4], PAIRS[(i + 2) % 4]):
            cands = [[clip, st, n] + trace(hits, s["uuids"][clip], nrows[clip], st, max_gap)
                     for (clip, st), n in sorted(named.items())]
            assert all(c[4] >= 1 for c in cands)  # a row's aligned_count >= 1: its diagonal has a hit
            occ, low, sup = occurrences(cands, s["uuids"], min_hits)
            per.append([max_gap, min_hits, cands, occ])
            seen["joined"] += sum(o[7] >= 2 for o in occ)
            seen["split"] += sum(c[5] >= 2 and c[6] < c[4] for c in cands)
            seen["suppressed"] += sup
            seen["low"] += low
            seen["occ"] += len(occ)
        out.append([name, qi, window, hop, ctx, per])
    # no empty shell
    assert seen["joined"] >= 1, seen      # an occurrence named by two windows or more
    assert seen["split"] >= 1, seen       # a trace of several segments, the best short of all the hits
    assert seen["suppressed"] >= 1, seen  # a candidate removed by suppression
    assert seen["low"] >= 1, seen         # a candidate dropped by min_hits
    assert {scen[c[0]]["queries"][c[1]]["coefs"] for c in out} == {1, 2}
    assert {c[4] < 0 for c in out} == {True, False}
    doc = {"generator": "tests/golden/make_golden_occurrences.py",
           "source": ["tests/golden/match_cases.json", "tests/golden/sliding_cases.json",
                      "tests/golden/sliding_aligned_cases.json"], "pairs": PAIRS, "cases": out}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("occurrence_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    doc = json.loads(text)
    print("wrote", PATH, "cases", len(doc["cases"]), "traces", sum(len(p[2]) for c in doc["cases"] for p in c[5]),
          "occurrences", sum(len(p[3]) for c in doc["cases"] for p in c[5]), "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
