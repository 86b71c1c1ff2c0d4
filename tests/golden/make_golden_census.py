"""Generate tests/golden/census_cases.json — how the reference's result set is distributed by count.

The reference's result query, "select *, count(*) from temp group by audio_uuid order by count(*) DESC"
(fp_handler.c:367-374), yields one row per clip with a non-zero count; the census of a query is
"select c, count(*) from (select count(*) c from temp group by audio_uuid) group by c": the number of
clips at each count. This fixture records it for every query of every scenario of match_cases.json
(none dropped), over all clips and over each of the three contexts of make_golden_scoped.py, derived
from the unmodified SqlFingerprintDB (oracle/sql_oracle.py) by peeling to exhaustion as
make_golden_ranked.py peels to row 7: search(), record the winner's count, delete the winner with the
reference's own statement (fp_handler.c:147), search again, until search() returns None.

The file holds only (scenario name, query index, [census over all clips, of ctx0, of ctx1, of ctx2])
with census = [[count, clips], ...], non-zero bins only, counts descending. Clips with count 0 never
appear in the result set; their number is the table's clip population minus the listed clips.

Run:  python tests/golden/make_golden_census.py            (writes the file)
      python tests/golden/make_golden_census.py --check    (exit 1 unless the file is reproduced byte for byte)
"""
from __future__ import annotations

import concurrent.futures
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, HERE)
from sql_oracle import SqlFingerprintDB  # noqa: E402

from make_golden_ranked import clip_rows  # noqa: E402
from make_golden_scoped import CONTEXTS, context_of  # noqa: E402

PATH = os.path.join(HERE, "census_cases.json")


def peel_census(s, x, qis=None):
    """Per query of scenario s (qis: of those queries) the census over the clips of context x (None: every clip)."""
    rows = clip_rows(s)
    col = {u: c for c, u in enumerate(s["uuids"]) if x is None or context_of(c) == "ctx%d" % x}
    db = SqlFingerprintDB()
    for u, c in col.items():
        db.insert_rows(context_of(c), u, rows[c][0], rows[c][1])
    out = []
    for q in (s["queries"] if qis is None else [s["queries"][i] for i in qis]):
        census, gone = [], []
        while True:
            res = db.search(q["q1"], q["q2"], q["coefs"], q["tol"], q["low"], q["high"])
            if res is None:
                break
            n = res["match_count"]
            assert not census or n <= census[-1][0]  # the result set's order: counts never rise
            if census and census[-1][0] == n:
                census[-1][1] += 1
            else:
                census.append([n, 1])
            db.db.execute("delete from audio_fingerprint where audio_uuid='%s';" % res["audio_uuid"])
            db.db.commit()
            gone.append(res["audio_uuid"])
        assert len(gone) == len(set(gone))
        for u in gone:  # the table again for the next query
            db.insert_rows(context_of(col[u]), u, rows[col[u]][0], rows[col[u]][1])
        out.append(census)
    return out


def _job(args):
    s, x, qis = args
    return peel_census(s, x, qis)


def generate() -> str:
    with open(os.path.join(HERE, "match_cases.json")) as f:
        cases = json.load(f)
    # one job per (scenario, table); a scenario of many clips (tie_2000) one per query as well: the
    # peels are independent, and the output does not depend on how they are spread over processes
    jobs = []
    for si, s in enumerate(cases["scenarios"]):
        for t in range(1 + CONTEXTS):
            x = None if t == 0 else t - 1
            if len(s["uuids"]) > 100:
                jobs += [(si, t, [qi], (s, x, [qi])) for qi in range(len(s["queries"]))]
            else:
                jobs.append((si, t, list(range(len(s["queries"]))), (s, x, None)))
    jobs.sort(key=lambda j: -len(j[3][0]["uuids"]) * len(j[2]))  # the long peels first
    workers = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count() or 1))
    if workers > 1:
        with concurrent.futures.ProcessPoolExecutor(workers) as pool:
            done = list(pool.map(_job, [j[3] for j in jobs], chunksize=1))
    else:
        done = [_job(j[3]) for j in jobs]
    per = {}
    for (si, t, qis, _), res in zip(jobs, done):
        for qi, cen in zip(qis, res):
            per[(si, qi, t)] = cen
    queries = []
    for si, s in enumerate(cases["scenarios"]):
        for qi in range(len(s["queries"])):
            queries.append([s["name"], qi, [per[(si, qi, t)] for t in range(1 + CONTEXTS)]])
    doc = {"generator": "tests/golden/make_golden_census.py", "source": "tests/golden/match_cases.json",
           "contexts": ["ctx%d" % x for x in range(CONTEXTS)], "queries": queries}
    return json.dumps(doc, separators=(",", ":")) + "\n"


def main():
    text = generate()
    if "--check" in sys.argv[1:]:
        with open(PATH) as f:
            same = f.read() == text
        print("census_cases.json", "reproduced" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write(text)
    doc = json.loads(text)
    n = sum(sum(k for _, k in q[2][0]) for q in doc["queries"])
    print("wrote", PATH, "queries", len(doc["queries"]), "clips counted over all clips", n, "bytes", os.path.getsize(PATH))


if __name__ == "__main__":
    main()
