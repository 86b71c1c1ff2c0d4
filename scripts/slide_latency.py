"""Latency of sliding search against the same windows cut on the host and sent through ranked search.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000), then
times, in one process through the same Python call path, on one 60 s 8 kHz recording (1,875 frames:
noise, a 20 s excerpt of a DB clip, noise), window 94 frames, hop in {1, 8, 94}, k in {1, 8}, coefs = 1,
tolerance 0.001: tfp_search_sliding_pcm_batch, and the explicit form: the windows' samples cut out on
the host (before the clock starts) and passed to tfp_search_ranked_pcm_batch as one batch of queries.
p50 / p99 over --calls calls after --warmup, and the ratio sliding p50 / explicit p50 of each shape.
Then a batch of --batch such recordings (default 64) at hop 8, k 8, both ways, best of 3. Writes
profiles/slide_latency.json and prints it. Run it under a time limit of its own:

    timeout 900 python scripts/slide_latency.py
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

WINDOW = 94
SECONDS = 60


def pct(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e6, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slide_latency.json"))
    args = ap.parse_args()
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    rng = np.random.default_rng(bench.SEED_Q)
    n = 8000 * SECONDS

    def recording(i):
        c = int(rng.integers(args.db_clips))
        rec = T.synth_pcm(0xBEEF, [i], n)[0].copy()
        rec[256 * 600:256 * 600 + 8000 * 20] = T.synth_pcm(bench.SEED_DB, [c], 8000 * 20, offsets=[256 * 100])[0]
        return rec, c

    rec, _ = recording(0)
    off = np.array([0, n], np.int64)
    p = T.params(1, 0.001)
    nf = T.frame_count(n)

    def timed(call):
        ts = []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                ts.append(dt)
        return {"p50_us": pct(ts, 50), "p99_us": pct(ts, 99)}

    def cuts(recs, hop):
        nw = T.sliding_windows(nf, WINDOW, hop)
        flat = np.concatenate([r[w * hop * 256:(w * hop + WINDOW) * 256] for r in recs for w in range(nw)])
        return flat, np.arange(len(recs) * nw + 1, dtype=np.int64) * (WINDOW * 256), nw

    res = {"workload": f"one {SECONDS} s 8 kHz recording ({nf} frames), window {WINDOW}, vs {args.db_clips} x 30 s clips, "
                       "coefs 1, tolerance 0.001",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for hop in (1, 8, 94):
        flat, qoff, nw = cuts([rec], hop)
        for k in (1, 8):
            s = timed(lambda: eng.search_sliding_pcm_batch(rec, off, p, WINDOW, hop, k))
            e = timed(lambda: eng.search_ranked_pcm_batch(flat, qoff, p, k))
            key = "hop%d_k%d" % (hop, k)
            res[key] = {"windows": nw, "sliding": s, "explicit": e, "sliding_to_explicit_p50": s["p50_us"] / e["p50_us"]}
        # (the two forms' rows differ only through each cut's frame 0, which sees zero history)
        assert len(eng.search_sliding_pcm_batch(rec, off, p, WINDOW, hop, 1)[0]) == nw == len(qoff) - 1
    hop, k = 8, 8
    recs = [recording(i)[0] for i in range(args.batch)]
    many = np.concatenate(recs)
    moff = np.arange(args.batch + 1, dtype=np.int64) * n
    flat, qoff, nw = cuts(recs, hop)
    big = {"recordings": args.batch, "hop": hop, "k": k, "windows": args.batch * nw}
    for name, call in (("sliding", lambda: eng.search_sliding_pcm_batch(many, moff, p, WINDOW, hop, k)),
                       ("explicit", lambda: eng.search_ranked_pcm_batch(flat, qoff, p, k))):
        call()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        big[name + "_call_ms"] = best * 1e3
    big["sliding_to_explicit"] = big["sliding_call_ms"] / big["explicit_call_ms"]
    res["batch_%d" % args.batch] = big
    res["slide_stats"] = eng.slide_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
