"""Generate tests/golden/scoped_cases.json — the first rows of the reference's result set per context.

The reference's documentation promises a search within the caller's context
(doc/dialplan_application.rst:11, :52-53); its per-frame insert (fp_handler.c:308-314) has no context
predicate. With "and context = '<ctx>'" added there, the result query (fp_handler.c:367-374) sees the
rows of that context's clips only, which is the unmodified SQL over a table that holds only those
clips. This fixture records exactly that: per context an unmodified SqlFingerprintDB
(oracle/sql_oracle.py) holding only the context's clips, peeled as make_golden_ranked.py peels the
whole table (search(), record the winner, delete it with the reference's own statement,
fp_handler.c:147, search again) to rows 0..7.

Clip c of a scenario is in context "ctx%d" % (c % 3), as make_golden_ranked.py inserts them. Every
query of every scenario of match_cases.json is peeled in each of the three contexts (none dropped).
The file holds only (scenario name, query index, [rows of ctx0, rows of ctx1, rows of ctx2]) with
rows = [[clip, match_count], ...], clip being the index of the row's audio_uuid in the scenario's
"uuids" list of match_cases.json (a sixth of the bytes of the uuid strings).

Run:  python tests/golden/make_golden_scoped.py            (writes the file)
      python tests/golden/make_golden_scoped.py --check    (exit 1 unless the file is reproduced byte for byte)
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

RANKS = 8
CONTEXTS = 3
PATH = os.path.join(HERE, "scoped_cases.json")


def context_of(c: int) -> str:
    return "ctx%d" % (c % CONTEXTS)


def peel_context(s, x):
    """Per query of scenario s the peeled rows over the clips of context x alone."""
    rows = clip_rows(s)
    ctx = "ctx%d" % x
    col = {u: c for c, u in enumerate(s["uuids"]) if context_of(c) == ctx}
    db = SqlFingerprintDB()
    for u, c in col.items():
        db.insert_rows(ctx, u, rows[c][0], rows[c][1])
    out = []
    for q in s["queries"]:
        ranked, gone = [], []
        while len(ranked) < RANKS:
            res = db.search(q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"])
            if res is None:
                break
            ranked.append([col[res["audio_uuid"]], res["match_count"]])
            db.db.execute("delete from audio_fingerprint where audio_uuid='%s';" % res["audio_uuid"])
            db.db.commit()
            gone.append(res["audio_uuid"])
        for u in gone:  # the context's table again for the next query
            db.insert_rows(ctx, u, rows[col[u]][0], rows[col[u]][1])
        out.append(ranked)
    return out


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        cases = json.load(f)
    queries = []
    for s in cases["scenarios"]:
        per_ctx = [peel_context(s, x) for x in range(CONTEXTS)]
        for qi in range(len(s["queries"])):
            queries.append([s["name"], qi, [per_ctx[x][qi] for x in range(CONTEXTS)]])
    doc = {"generator": "tests/golden/make_golden_scoped.py", "source": "tests/golden/match_cases.json",
           "ranks": RANKS, "contexts": ["ctx%d" % x for x in range(CONTEXTS)], "queries": queries}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("scoped_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    doc = json.loads(text)
    n = sum(1 for q in doc["queries"] for rows in q[2] if rows)
    print("wrote", PATH, "queries", len(doc["queries"]), "context lists with rows", n, "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
