"""Generate tests/golden/aligned_cases.json — where in each candidate clip a golden query matches.

For every query of match_cases.json and rows 0..2 of its ranked result (ranked_cases.json), the
alignment of (query, clip): with hit(i, j) = "query frame i runs its SQL and the clip's stored row j
(frame_idx j) satisfies its predicate" and hist[d] = #{(i, j) : hit(i, j), j - i = d},
    aligned_count = max hist, offset = the smallest d attaining it,
    first_frame / last_frame = the least / greatest i with hit(i, i + offset); all 0 when nothing hits.

The hits come from SQLite, not numpy: per query frame the reference's own predicate text
(fp_handler.c:287-351, the literals as oracle/sql_oracle.py formats them, the frame skipped where the
reference skips it or its SQL fails) runs as
    select frame_idx from audio_fingerprint where audio_uuid='...' and <predicate>
against the scenario's table, which oracle/sql_oracle.py's insert_rows fills with one row per frame and
its frame_idx. The histogram over frame_idx - i is then plain Python. No query is dropped.

The file holds only (scenario name, query index, row, uuid, aligned_count, offset, first_frame,
last_frame).

Run:  python tests/golden/make_golden_aligned.py            (writes the file)
      python tests/golden/make_golden_aligned.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import json
import math
import os
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from sql_oracle import SqlFingerprintDB, _f  # noqa: E402

ROWS = 3
PATH = os.path.join(HERE, "aligned_cases.json")


def frame_predicate(v1, v2, coefs, tole, low, high):
    """The where clause fp_search_fingerprint_info builds for one query frame (fp_handler.c:287-351, as
    SqlFingerprintDB.search words it), or None where the frame runs no SQL."""
    v1 = v1 if v1 is not None else 0.0  # ast_json_real_get(NULL) == 0.0
    freq = float(int(v1))               # (int) truncation, fp_handler.c:290
    if low > 0 and freq < 10 * math.log10(low):
        return None
    if high > 0 and freq > 10 * math.log10(high):
        return None
    sql = " max1 >= %s  and max1 <= %s " % (_f(freq - tole), _f(freq + tole))
    for j in range(1, coefs):
        v = v2 if v2 is not None else 0.0
        if low > 0 and v < 10 * math.log10(low):
            continue
        if high > 0 and v > 10 * math.log10(high):
            continue
        sql = "%s and max%d >= %s and max%d <= %s" % (sql, j + 1, _f(v - tole), j + 1, _f(v + tole))
    return sql


def align(db, uuid, q):
    """(aligned_count, offset, first_frame, last_frame) of query q against clip uuid."""
    tole = q["tol"]
    if tole < 0:  # fp_handler.c:252-256 (a NaN tolerance stays: its SQL fails, frame by frame)
        tole = 0.001
    hist, on = {}, {}
    for i, (v1, v2) in enumerate(zip(q["q1"], q["q2"])):
        pred = frame_predicate(v1, v2, q["coefs"], tole, q["low"], q["high"])
        if pred is None:
            continue
        try:
            rows = db.db.execute("select frame_idx from audio_fingerprint where audio_uuid='%s' and %s" % (uuid, pred)).fetchall()
        except sqlite3.Error:
            continue  # the reference's insert fails the same way and its loop goes on (fp_handler.c:357-359)
        for (j,) in rows:
            d = j - i
            hist[d] = hist.get(d, 0) + 1
            on.setdefault(d, []).append(i)
    if not hist:
        return [0, 0, 0, 0]
    best = max(hist.values())
    off = min(d for d, n in hist.items() if n == best)
    return [best, off, min(on[off]), max(on[off])]


def clip_rows(s):
    rows = [([], []) for _ in s["uuids"]]
    for c, a, b in zip(s["clip"], s["m1"], s["m2"]):
        rows[c][0].append(a)
        rows[c][1].append(b)
    return rows


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        cases = json.load(f)
    with open(os.path.join(HERE, "ranked_cases.json")) as f:
        ranked = {(name, qi): rows for name, qi, rows in json.load(f)["queries"]}
    pairs = []
    for s in cases["scenarios"]:
        db = SqlFingerprintDB()
        for c, (m1s, m2s) in enumerate(clip_rows(s)):
            db.insert_rows("ctx%d" % (c % 3), s["uuids"][c], m1s, m2s)
        for qi, q in enumerate(s["queries"]):
            for r, (uuid, _count) in enumerate(ranked[(s["name"], qi)][:ROWS]):
                pairs.append([s["name"], qi, r, uuid] + align(db, uuid, q))
    doc = {"generator": "tests/golden/make_golden_aligned.py",
           "source": ["tests/golden/match_cases.json", "tests/golden/ranked_cases.json"], "rows": ROWS, "pairs": pairs}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("aligned_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    print("wrote", PATH, "pairs", len(json.loads(text)["pairs"]), "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
