"""Generate tests/golden/sliding_aligned_cases.json — where in its clip each row of each window of a
recording matches.

For every case of sliding_cases.json (a query of match_cases.json taken as the recording, a window, a
hop, a context), every window w of it and rows 0 and 1 of that window's result, the alignment of
(the window's frames [w * hop, w * hop + window) alone, the row's clip), exactly as
make_golden_aligned.py computes it for a whole query: the hits come from SQLite, per window frame the
reference's own predicate text (fp_handler.c:287-351) run as
    select frame_idx from audio_fingerprint where audio_uuid='...' and <predicate>
against the scenario's table, and the histogram over frame_idx - i (i counted from the window's first
frame) is plain Python: aligned_count = its maximum, offset = the smallest diagonal attaining it,
first_frame / last_frame = the least / greatest window frame that hits on it.

The 48 committed cases alone (659 windows, 571 entries) miss one assertion below: 184 entries have
aligned_count < match_count, short of a third, because half the cases have window 1 or 4, where a
clip's few hits nearly always share a diagonal. So the generator adds windows and hops of its own,
not sliding_cases.json's: for each case with window 1 the same recording and context at window 8,
hop 2, and for each with window 4 at window 12, hop 5, their rows peeled as make_golden_sliding.py
peels them (peel_case, rows 0..1 kept). With them every assertion holds.

The file holds "cases": in sliding_cases.json's case order, (scenario name, query index, window, hop,
context or -1, [per window [[aligned_count, offset, first_frame, last_frame] for rows 0..1]]), and
"extra": the added cases in the same form with each row as [clip, match_count, aligned_count, offset,
first_frame, last_frame], clip being the index of the row's audio_uuid in the scenario's "uuids".

Run:  python tests/golden/make_golden_sliding_aligned.py            (writes the file)
      python tests/golden/make_golden_sliding_aligned.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, HERE)
from sql_oracle import SqlFingerprintDB  # noqa: E402

from make_golden_aligned import align, clip_rows  # noqa: E402
from make_golden_sliding import peel_case  # noqa: E402

ROWS = 2
EXTRA = {1: (8, 2), 4: (12, 5)}  # a committed case's window -> the added case's (window, hop)
PATH = os.path.join(HERE, "sliding_aligned_cases.json")


def shape(cases, sliding):
    """(entries, entries with aligned_count < match_count, cases where one clip keeps offset - w * hop
    over two consecutive windows)."""
    n = below = joined = 0
    for (_, _, _, hop, _, wins), (_, _, _, _, _, swins) in zip(cases, sliding):
        seen = False
        for w, (fours, rows) in enumerate(zip(wins, swins)):
            for four, (_clip, count) in zip(fours, rows):
                n += 1
                below += four[0] < count
            if w and not seen:
                prev = {c: f[1] - (w - 1) * hop for f, (c, _) in zip(wins[w - 1], swins[w - 1]) if f[0]}
                seen = any(f[0] and prev.get(c) == f[1] - w * hop for f, (c, _) in zip(fours, rows))
        joined += seen
    return n, below, joined


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        scen = {s["name"]: s for s in json.load(f)["scenarios"]}
    with open(os.path.join(HERE, "sliding_cases.json")) as f:
        sliding = json.load(f)["cases"]
    out, rows_of, dbs = [], [], {}
    todo = [c + [False] for c in sliding]
    for name, qi, window, hop, ctx, _wins in sliding:
        if window in EXTRA and len(scen[name]["queries"][qi]["q1"]) >= EXTRA[window][0]:
            w2, h2 = EXTRA[window]
            wins = [rows[:ROWS] for rows in peel_case(scen[name], qi, w2, h2, ctx)]
            todo.append([name, qi, w2, h2, ctx, wins, True])
    for name, qi, window, hop, ctx, wins, _extra in todo:
        s = scen[name]
        if name not in dbs:  # every clip: the alignment names its clip, whatever the case's context
            dbs = {name: SqlFingerprintDB()}
            for c, (m1s, m2s) in enumerate(clip_rows(s)):
                dbs[name].insert_rows("ctx%d" % (c % 3), s["uuids"][c], m1s, m2s)
        q = s["queries"][qi]
        per = []
        for w, rows in enumerate(wins):
            cut = dict(q, q1=q["q1"][w * hop:w * hop + window], q2=q["q2"][w * hop:w * hop + window])
            assert len(cut["q1"]) == window
            per.append([align(dbs[name], s["uuids"][c], cut) for c, _count in rows[:ROWS]])
        out.append([name, qi, window, hop, ctx, per])
        rows_of.append([name, qi, window, hop, ctx, wins])
    ncom = len(sliding)
    assert ncom == 48 and sum(len(c[5]) for c in out[:ncom]) == 659, (ncom, sum(len(c[5]) for c in out[:ncom]))
    n, below, joined = shape(out, rows_of)
    assert 3 * below >= n > 0, (below, n)  # no empty shell: the hits that line up are fewer than the hits
    assert joined >= 1, joined             # and a clip keeps its place from one window to the next
    assert {scen[c[0]]["queries"][c[1]]["coefs"] for c in out} == {1, 2}
    assert {c[4] < 0 for c in out} == {True, False}
    extra = [c[:5] + [[[list(r) + f for r, f in zip(rows, fours)] for rows, fours in zip(ro[5], c[5])]]
             for c, ro in zip(out[ncom:], rows_of[ncom:])]
    doc = {"generator": "tests/golden/make_golden_sliding_aligned.py",
           "source": ["tests/golden/match_cases.json", "tests/golden/sliding_cases.json"], "rows": ROWS, "cases": out[:ncom], "extra": extra}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("sliding_aligned_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    doc = json.loads(text)
    print("wrote", PATH, "cases", len(doc["cases"]), "extra", len(doc["extra"]), "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
