"""Batch-1 latency of aligned search against ranked search on the bench's synthetic DB, and one large
batch of the align launch.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000), then
times tfp_search_aligned_batch at k = 1, 8, 32 (coefs = 1, tolerance 0.001) and, in the same process
through the same Python call path, tfp_search_ranked_batch at the same k on the same 5 s query frames:
p50 / p99 over --calls calls after --warmup, and the ratio aligned / ranked (the ctypes overhead is in
both). Then one batch of --batch queries (default 4,096) at k = 8 through tfp_align_batch alone, with
the ids a ranked search returned: its wall time (best of 3 after a warm-up call, host clock around a
call that ends in a device synchronise) and the box tests per second, counted from the shapes as the
sum over the pairs of frames x rows. Writes profiles/align_latency.json and prints it. Run it under a
time limit of its own:

    timeout 900 python scripts/align_latency.py
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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "align_latency.json"))
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
    rows_per_clip = T.frame_count(n_db)
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
    for k in (1, 8, 32):
        r = timed(lambda fr, k=k: eng.search_ranked_batch(fr, [0, len(fr)], p, k))
        a = timed(lambda fr, k=k: eng.search_aligned_batch(fr, [0, len(fr)], p, k))
        a["p50_ratio_to_ranked"] = a["p50_us"] / r["p50_us"]
        res["ranked_k%d" % k], res["aligned_k%d" % k] = r, a
    res["ranked_k1_again"] = timed(lambda fr: eng.search_ranked_batch(fr, [0, len(fr)], p, 1))  # (drift check)
    # the aligned rows are the ranked rows, and every aligned count is within its match count
    for fr in queries:
        a = eng.search_aligned_batch(fr, [0, len(fr)], p, 8)[0]
        b = eng.search_ranked_batch(fr, [0, len(fr)], p, 8)[0]
        assert [{f: r[f] for f in c} for r, c in zip(a, b)] == b and len(a) == len(b)
        assert all(1 <= r["aligned_count"] <= r["match_count"] for r in a)
    res["aligned_rows_k8"] = [eng.search_aligned_batch(fr, [0, len(fr)], p, 8)[0][:2] for fr in queries[:3]]

    # one large batch of the align launch alone
    nb, k = args.batch, 8
    frames = np.concatenate([queries[i % len(queries)] for i in range(nb)])
    qoff = np.concatenate([[0], np.cumsum([len(queries[i % len(queries)]) for i in range(nb)])])
    ranked = eng.search_ranked_batch(frames, qoff, p, k)
    ids = np.full((nb, k), -1, np.int32)
    tests = 0
    for q, rows in enumerate(ranked):
        for r, row in enumerate(rows):
            ids[q, r] = row["clip_id"]
            tests += int(qoff[q + 1] - qoff[q]) * rows_per_clip
    eng.align_batch(frames, qoff, p, ids, k)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        eng.align_batch(frames, qoff, p, ids, k)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    res["align_batch"] = {"queries": nb, "k": k, "pairs": int((ids >= 0).sum()), "box_tests": tests, "call_ms": best * 1e3,
                          "box_tests_per_s": tests / best,
                          "note": "wall time of tfp_align_batch: frame upload, boxes, align launch, merge, copy back"}
    res["align_stats"] = eng.align_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
