"""Batch-1 latency of scoped search against ranked search on the bench's synthetic DB, one large scoped
batch, and an enrolment followed by a scoped search.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000), then
times, in one process through the same Python call path, on the same 5 s query frames (coefs = 1,
tolerance 0.001), at k = 1 and 8: tfp_search_ranked_batch; tfp_search_scoped_batch with every clip in one
scope (the query in that scope); and the same with the clips in 16 equal scopes (clip c in scope c % 16,
the query in the scope of its source clip). p50 / p99 over --calls calls after --warmup, and the ratio
of each scoped p50 to the ranked p50 of the same k. Then one batch of --batch queries (default 4,096) at
k = 8, ranked and scoped over the 16 scopes (wall time of the call, best of 3), and the p50 of "enrol
one clip, set its scope, scoped search" over --enrols rounds (each round pays the index delta's update
and one build of the scope table). Writes profiles/scope_latency.json and prints it. Run it under a time
limit of its own:

    timeout 900 python scripts/scope_latency.py
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
    ap.add_argument("--enrols", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scope_latency.json"))
    args = ap.parse_args()
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    rng = np.random.default_rng(bench.SEED_Q)
    qn, n_db = 8000 * 5, 8000 * 30
    queries, sources = [], []
    for i in range(8):  # 5 s excerpts of DB clips at hop-aligned offsets
        c = int(rng.integers(args.db_clips))
        pcm = T.synth_pcm(bench.SEED_DB, [c], qn, offsets=[256 * int(rng.integers(0, (n_db - qn) // 256))])[0]
        queries.append(eng.fingerprint(pcm))
        sources.append(c)
    p = T.params(1, 0.001)

    def timed(call):
        ts = []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            call(i % len(queries))
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                ts.append(dt)
        return {"p50_us": pct(ts, 50), "p99_us": pct(ts, 99)}

    res = {"workload": f"batch-1 5 s query frames vs {args.db_clips} x 30 s clips, coefs 1, tolerance 0.001",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    all_uuids = [bench.uuid_of(c) for c in range(args.db_clips)]
    clip_of = {u: c for c, u in enumerate(all_uuids)}
    for layout, scope_of in (("one_scope", lambda c: 1), ("sixteen_scopes", lambda c: 1 + c % SCOPES)):
        eng.index_set_scope(all_uuids, [scope_of(c) for c in range(args.db_clips)])
        qscope = [scope_of(c) for c in sources]
        for k in (1, 8):
            r = timed(lambda i, k=k: eng.search_ranked_batch(queries[i], [0, len(queries[i])], p, k))
            s = timed(lambda i, k=k: eng.search_scoped_batch(queries[i], [0, len(queries[i])], p, [qscope[i]], k))
            s["p50_ratio_to_ranked"] = s["p50_us"] / r["p50_us"]
            res["%s_ranked_k%d" % (layout, k)], res["%s_scoped_k%d" % (layout, k)] = r, s
        # the scoped rows are the ranked rows of the scope's clips
        for i, fr in enumerate(queries):
            got = eng.search_scoped_batch(fr, [0, len(fr)], p, [qscope[i]], 8)[0]
            want = [r for r in eng.search_ranked_batch(fr, [0, len(fr)], p, 32)[0]
                    if scope_of(clip_of[r["audio_uuid"]]) == qscope[i]][:8]
            assert got[:len(want)] == want, (layout, i)
    # one large batch, the 16 scopes standing
    nb, k = args.batch, 8
    frames = np.concatenate([queries[i % len(queries)] for i in range(nb)])
    qoff = np.concatenate([[0], np.cumsum([len(queries[i % len(queries)]) for i in range(nb)])])
    bscope = [1 + sources[i % len(queries)] % SCOPES for i in range(nb)]
    big = {}
    for name, call in (("ranked", lambda: eng.search_ranked_batch(frames, qoff, p, k)),
                       ("scoped", lambda: eng.search_scoped_batch(frames, qoff, p, bscope, k))):
        call()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        big[name + "_call_ms"] = best * 1e3
    big["scoped_ratio_to_ranked"] = big["scoped_call_ms"] / big["ranked_call_ms"]
    res["batch_%d_k8" % nb] = big
    # enrol one clip, set its scope, scoped search
    ts = []
    fr0 = queries[0]
    for j in range(args.enrols):
        u = "ffffffff-0000-4000-8000-%012d" % j
        t0 = time.perf_counter()
        eng.index_add(u, fr0["m1"], fr0["m2"])
        eng.index_set_scope([u], [1 + j % SCOPES])
        eng.search_scoped_batch(fr0, [0, len(fr0)], p, [1 + j % SCOPES], 1)
        ts.append(time.perf_counter() - t0)
    res["enrol_then_scoped_search"] = {"rounds": args.enrols, "p50_us": pct(ts, 50), "p99_us": pct(ts, 99),
                                       "delta_clips": eng.index_delta_stats()[1]}
    res["scope_stats"] = eng.scope_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
