"""Latency of the match census against scoped search on the bench's synthetic DB: one large batch and
batch-1.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000) with
the clips in 16 equal scopes, then times, in one process through the same Python call path, on the same
5 s query frames (coefs = 1, tolerance 0.001): tfp_census_batch, and tfp_search_scoped_batch at k = 1
and k = 32, with the three calls' repetitions interleaved. Batch-1: p50 / p99 over --calls rounds after
--warmup. One batch of --batch queries (default 4,096): the wall time of the call, best of --reps. The
ratios of the census to each scoped time go into the file; nothing is gated on them. The census rows
are checked against the scoped rows on the way (the k = 32 counts are the census read from the top).
Writes profiles/census_latency.json and prints it. Run it under a time limit of its own:

    timeout 900 python scripts/census_latency.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "asterisk-tiresias_amd"))

SCOPES = 16


def pct(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e6, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "census_latency.json"))
    args = ap.parse_args()
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    eng.index_set_scope([bench.uuid_of(c) for c in range(args.db_clips)], [1 + c % SCOPES for c in range(args.db_clips)])
    rng = np.random.default_rng(bench.SEED_Q)
    qn, n_db = 8000 * 5, 8000 * 30
    queries, qscope = [], []
    for i in range(8):  # 5 s excerpts of DB clips at hop-aligned offsets
        c = int(rng.integers(args.db_clips))
        pcm = T.synth_pcm(bench.SEED_DB, [c], qn, offsets=[256 * int(rng.integers(0, (n_db - qn) // 256))])[0]
        queries.append(eng.fingerprint(pcm))
        qscope.append(1 + c % SCOPES if i % 2 else -1)  # the source clip's scope, or every clip
    p = T.params(1, 0.001)
    res = {"workload": f"5 s query frames vs {args.db_clips} x 30 s clips in {SCOPES} scopes, coefs 1, tolerance 0.001; "
                       "queries alternate between every clip and one scope",
           "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    # the census agrees with the rows it is compared with
    for i, fr in enumerate(queries):
        row = eng.census_batch(fr, [0, len(fr)], p, [qscope[i]])[0]
        counts = [r["match_count"] for r in eng.search_scoped_batch(fr, [0, len(fr)], p, [qscope[i]], 32)[0]]
        assert counts == [c for c in range(len(row) - 1, 0, -1) for _ in range(row[c])][:32], i
    res["clips_at_winner_count"] = []  # per query: the clips that reach the winner's count (0: no clip was hit)
    for fr, s in zip(queries, qscope):
        top = eng.search_scoped_batch(fr, [0, len(fr)], p, [s], 1)[0]
        row = eng.census_batch(fr, [0, len(fr)], p, [s])[0]
        res["clips_at_winner_count"].append(int(T.census_at_least(row, top[0]["match_count"])) if top else 0)

    calls = {"census": lambda fr, qo, sc: eng.census_batch(fr, qo, p, sc),
             "scoped_k1": lambda fr, qo, sc: eng.search_scoped_batch(fr, qo, p, sc, 1),
             "scoped_k32": lambda fr, qo, sc: eng.search_scoped_batch(fr, qo, p, sc, 32)}
    # batch-1, the three calls interleaved round by round
    ts = {name: [] for name in calls}
    for i in range(args.warmup + args.calls):
        fr, sc = queries[i % len(queries)], [qscope[i % len(queries)]]
        for name, call in calls.items():
            t0 = time.perf_counter()
            call(fr, [0, len(fr)], sc)
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                ts[name].append(dt)
    one = {name: {"p50_us": pct(v, 50), "p99_us": pct(v, 99)} for name, v in ts.items()}
    for k in ("scoped_k1", "scoped_k32"):
        one["census_p50_ratio_to_" + k] = one["census"]["p50_us"] / one[k]["p50_us"]
    res["batch_1"] = one
    # one large batch, interleaved repetitions, best of --reps
    nb = args.batch
    frames = np.concatenate([queries[i % len(queries)] for i in range(nb)])
    qoff = np.concatenate([[0], np.cumsum([len(queries[i % len(queries)]) for i in range(nb)])])
    bscope = [qscope[i % len(queries)] for i in range(nb)]
    best = {name: None for name in calls}
    for rep in range(args.reps + 1):  # (the first repetition warms up)
        for name, call in calls.items():
            t0 = time.perf_counter()
            call(frames, qoff, bscope)
            dt = time.perf_counter() - t0
            if rep:
                best[name] = dt if best[name] is None else min(best[name], dt)
    big = {name + "_call_ms": v * 1e3 for name, v in best.items()}
    for k in ("scoped_k1", "scoped_k32"):
        big["census_ratio_to_" + k] = best["census"] / best[k]
    res["batch_%d" % nb] = big
    res["census_stats"] = eng.census_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
