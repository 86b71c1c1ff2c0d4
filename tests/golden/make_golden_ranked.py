"""Generate tests/golden/ranked_cases.json — the first rows of the reference's result set.

The reference's result query, "select *, count(*) from temp group by audio_uuid order by count(*) DESC"
(fp_handler.c:367-374), yields a ranked list of clips of which the reference reads the first row. This
fixture records rows 0..7 for every query of match_cases.json, derived from the unmodified
SqlFingerprintDB (oracle/sql_oracle.py) by peeling: search(), record the winner, delete it with the
reference's own "delete from audio_fingerprint where audio_uuid='%s';" (fp_handler.c:147), search
again, until search() returns None or 8 rows are recorded. Row r of the result set is the winner once
rows 0..r-1 are gone: removing a clip leaves the other clips' counts as they were.

Every query of every scenario is peeled (none dropped). The file holds only
(scenario name, query index, [[uuid, match_count], ...]).

Run:  python tests/golden/make_golden_ranked.py            (writes the file)
      python tests/golden/make_golden_ranked.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from sql_oracle import SqlFingerprintDB  # noqa: E402

RANKS = 8
PATH = os.path.join(HERE, "ranked_cases.json")


def clip_rows(s):
    """Per clip the (m1s, m2s) of its rows in frame order."""
    rows = [([], []) for _ in s["uuids"]]
    for c, a, b in zip(s["clip"], s["m1"], s["m2"]):
        rows[c][0].append(a)
        rows[c][1].append(b)
    return rows


def peel_scenario(s):
    rows = clip_rows(s)
    col = {u: c for c, u in enumerate(s["uuids"])}
    db = SqlFingerprintDB()
    for c, u in enumerate(s["uuids"]):
        db.insert_rows("ctx%d" % (c % 3), u, rows[c][0], rows[c][1])
    out = []
    for qi, q in enumerate(s["queries"]):
        ranked, gone = [], []
        while len(ranked) < RANKS:
            res = db.search(q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"])
            if res is None:
                break
            ranked.append([res["audio_uuid"], res["match_count"]])
            db.db.execute("delete from audio_fingerprint where audio_uuid='%s';" % res["audio_uuid"])
            db.db.commit()
            gone.append(res["audio_uuid"])
        for u in gone:  # the scenario's table again for the next query
            c = col[u]
            db.insert_rows("ctx%d" % (c % 3), u, rows[c][0], rows[c][1])
        expect = q["expect"]
        assert (ranked[0] if ranked else None) == ([expect["audio_uuid"], expect["match_count"]] if expect else None)
        out.append(ranked)
    return out


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        cases = json.load(f)
    queries = []
    for s in cases["scenarios"]:
        for qi, ranked in enumerate(peel_scenario(s)):
            queries.append([s["name"], qi, ranked])
    doc = {"generator": "tests/golden/make_golden_ranked.py", "source": "tests/golden/match_cases.json",
           "ranks": RANKS, "queries": queries}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("ranked_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    n = sum(1 for q in json.loads(text)["queries"] if q[2])
    print("wrote", PATH, "queries", len(json.loads(text)["queries"]), "with rows", n, "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
