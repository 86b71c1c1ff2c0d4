"""Generate tests/golden/sliding_cases.json — the first rows of the reference's result set for every
window of a recording.

The reference searches one fixed window of audio (application_handler.c:152-185,
fp_handler.c:275-374). Sliding search runs the same result query (fp_handler.c:367-374) over the
frames [w * hop, w * hop + window) of a longer recording, for every w with a full window. This
fixture records exactly that with the unmodified SqlFingerprintDB (oracle/sql_oracle.py): a query of
match_cases.json taken as the recording, each window's frames searched on their own and peeled as
make_golden_ranked.py peels a query (search(), record the winner, delete it with the reference's own
statement, fp_handler.c:147, search again) to rows 0..3. A case with a context holds only that
context's clips in the table, as make_golden_scoped.py does (clip c in "ctx%d" % (c % 3)).

Cases: per scenario with clips, in file order, the eligible queries (at least 12 frames, coefs 1 or
2) are taken round robin, two per scenario, one of coefs 2 where the scenario has one; case number n
gets window (1, 4, 16, F)[n % 4], hop (1, 3, window, window + 2)[(n // 4) % 4] and context
(none, ctx0, ctx1, ctx2)[(n // 16 + n) % 4], so every (window, hop) pair and every context occurs.
The file holds (scenario name, query index, window, hop, context or -1, [per window [[clip,
match_count], ...]]), clip being the index of the row's audio_uuid in the scenario's "uuids".

Run:  python tests/golden/make_golden_sliding.py            (writes the file)
      python tests/golden/make_golden_sliding.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, HERE)
from sql_oracle import SqlFingerprintDB  # noqa: E402

from make_golden_ranked import clip_rows  # noqa: E402

RANKS = 4
CONTEXTS = 3
MIN_FRAMES = 12
PER_SCENARIO = 2
PATH = os.path.join(HERE, "sliding_cases.json")


def windows_of(nframes: int, window: int, hop: int) -> int:
    return 0 if nframes < window else (nframes - window) // hop + 1


def select(cases):
    """[(scenario, query index, window, hop, context or -1), ...], deterministic."""
    out = []
    for si, s in enumerate(cases["scenarios"]):
        if not s["uuids"]:
            continue
        ok = [qi for qi, q in enumerate(s["queries"]) if len(q["q1"]) >= MIN_FRAMES and q["coefs"] in (1, 2)]
        if not ok:
            continue
        two = [qi for qi in ok if s["queries"][qi]["coefs"] == 2]
        picks = [ok[si % len(ok)]]
        rest = [qi for qi in (two or ok) if qi not in picks] or ok
        picks.append(rest[(si // 2) % len(rest)])
        for qi in picks[:PER_SCENARIO]:
            n = len(out)
            F = len(s["queries"][qi]["q1"])
            window = (1, 4, 16, F)[n % 4]
            hop = (1, 3, window, window + 2)[(n // 4) % 4]
            out.append((s, qi, window, hop, (n // 16 + n) % 4 - 1))
    return out


def peel_case(s, qi, window, hop, ctx):
    """Per window of query qi of scenario s the peeled rows, over every clip (ctx -1) or context ctx's."""
    rows = clip_rows(s)
    col = {u: c for c, u in enumerate(s["uuids"]) if ctx < 0 or c % CONTEXTS == ctx}
    db = SqlFingerprintDB()
    for u, c in col.items():
        db.insert_rows("ctx%d" % (c % CONTEXTS), u, rows[c][0], rows[c][1])
    q = s["queries"][qi]
    out = []
    for w in range(windows_of(len(q["q1"]), window, hop)):
        q1, q2 = q["q1"][w * hop:w * hop + window], q["q2"][w * hop:w * hop + window]
        ranked, gone = [], []
        while len(ranked) < RANKS:
            res = db.search(q1, q2, q["coefs"], q["tol"], q["low"], q["high"])
            if res is None:
                break
            assert res["frame_count"] == window
            ranked.append([col[res["audio_uuid"]], res["match_count"]])
            db.db.execute("delete from audio_fingerprint where audio_uuid='%s';" % res["audio_uuid"])
            db.db.commit()
            gone.append(res["audio_uuid"])
        for u in gone:  # the table again for the next window
            db.insert_rows("ctx%d" % (col[u] % CONTEXTS), u, rows[col[u]][0], rows[col[u]][1])
        out.append(ranked)
    return out


def shape(cases):
    """(windows, windows with >= 2 rows, cases, cases whose winner changes between windows)."""
    wins = [w for c in cases for w in c[5]]
    moved = sum(1 for c in cases if len({w[0][0] if w else -1 for w in c[5]}) > 1)
    return len(wins), sum(1 for w in wins if len(w) >= 2), len(cases), moved


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        cases = json.load(f)
    out = [[s["name"], qi, window, hop, ctx, peel_case(s, qi, window, hop, ctx)] for s, qi, window, hop, ctx in select(cases)]
    nwin, deep, ncases, moved = shape(out)
    assert 3 * deep >= nwin > 0, (deep, nwin)      # no empty shell: the rows reach below the winner
    assert 5 * moved >= ncases > 0, (moved, ncases)  # and the winner moves along the recording
    assert {c[2] for c in out} >= {1, 4, 16} and {c[4] for c in out} == {-1, 0, 1, 2}
    assert {q_coefs(cases, c) for c in out} == {1, 2}
    doc = {"generator": "tests/golden/make_golden_sliding.py", "source": "tests/golden/match_cases.json",
           "ranks": RANKS, "contexts": ["ctx%d" % x for x in range(CONTEXTS)], "cases": out}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def q_coefs(cases, c):
    s = next(s for s in cases["scenarios"] if s["name"] == c[0])
    return s["queries"][c[1]]["coefs"]


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("sliding_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    print("wrote", PATH, "windows, deep, cases, moved", shape(json.loads(text)["cases"]), "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
