"""Batch-1 latency of ranked search against plain search on the bench's synthetic DB.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000),
then times tfp_search_ranked at k = 1, 8, 32 (coefs = 1, tolerance 0.001) and, in the same process
through the same Python call path, tfp_search on the same 5 s query frames: p50 / p99 over --calls
calls after --warmup, and the ratio ranked / plain (the ctypes overhead is in both). Writes
profiles/rank_latency.json and prints it. Run it under a time limit of its own:

    timeout 600 python scripts/rank_latency.py
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


def pct(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e6, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rank_latency.json"))
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
    queries = []
    for i in range(8):  # 5 s excerpts of DB clips at hop-aligned offsets (two of them unrelated audio)
        if i % 4 != 3:
            pcm = T.synth_pcm(bench.SEED_DB, [int(rng.integers(args.db_clips))], qn,
                              offsets=[256 * int(rng.integers(0, (n_db - qn) // 256))])[0]
        else:
            pcm = T.synth_pcm(bench.SEED_Q, [i], qn)[0]
        queries.append(eng.fingerprint(pcm))
    p = T.params(1, 0.001)

    def timed(call):
        ts = []
        for i in range(args.warmup + args.calls):
            fr = queries[i % len(queries)]
            t0 = time.perf_counter()
            call(fr)
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                ts.append(dt)
        return {"p50_us": pct(ts, 50), "p99_us": pct(ts, 99)}

    res = {"workload": f"batch-1 5 s query frames vs {args.db_clips} x 30 s clips, coefs 1, tolerance 0.001",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    res["plain"] = timed(lambda fr: eng.search(fr, p))
    rows = [len(eng.search_ranked(fr, p, 32)) for fr in queries]
    for k in (1, 8, 32):
        r = timed(lambda fr, k=k: eng.search_ranked(fr, p, k))
        r["p50_ratio_to_plain"] = r["p50_us"] / res["plain"]["p50_us"]
        res["ranked_k%d" % k] = r
    res["plain_again"] = timed(lambda fr: eng.search(fr, p))  # (drift check: the same figure after the ranked runs)
    res["rows_at_k32"] = rows
    res["rank_stats"] = eng.rank_stats()
    # row 0 is the plain search's answer
    for fr in queries:
        a, _ = eng.search(fr, p)
        b = eng.search_ranked(fr, p, 1)
        assert (None if a is None else (a["audio_uuid"], a["match_count"])) == \
            ((b[0]["audio_uuid"], b[0]["match_count"]) if b else None)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
