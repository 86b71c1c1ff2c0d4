"""Latency of sliding aligned search against the composition the engine offered before it: sliding
search, the windows cut on the host, aligned search on the cuts.

Enrols the match leg's synthetic index (bench.enroll: --db-clips x 30 s clips, default 100,000), then
times, in one process through the same Python call path, on one 60 s 8 kHz recording (1,875 frames:
noise, a 20 s excerpt of a DB clip, noise), window 94 frames, hop in {1, 8, 47}, k in {1, 8}, coefs = 1,
tolerance 0.001: tfp_search_sliding_aligned_pcm_batch, and the composition: tfp_search_sliding_pcm_batch,
then every window's frames cut out of the recording's fingerprint on the host (one numpy gather, inside the
clock: the caller has to do it per call), the clip ids read out of the sliding rows (a Python list per window,
as the binding returns dicts; the fused call's binding builds the same dicts) and tfp_align_batch. hop 1 and 8
take the slid form (2 * hop < window), hop 47 the direct form. p50 / p99 over --calls calls after --warmup, and
the ratio fused p50 / composed p50 of each shape. Writes profiles/slide_align_latency.json and prints
it. Run it under a time limit of its own:

    timeout 900 python scripts/slide_align_latency.py
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slide_align_latency.json"))
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
    c = int(rng.integers(args.db_clips))
    rec = T.synth_pcm(0xBEEF, [0], n)[0].copy()
    rec[256 * 600:256 * 600 + 8000 * 20] = T.synth_pcm(bench.SEED_DB, [c], 8000 * 20, offsets=[256 * 100])[0]
    off = np.array([0, n], np.int64)
    p = T.params(1, 0.001)
    nf = T.frame_count(n)
    frames = eng.fingerprint_batch(rec, off)  # (the composition's caller holds the recording's frames)

    def timed(call):
        ts = []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                ts.append(dt)
        return {"p50_us": pct(ts, 50), "p99_us": pct(ts, 99)}

    def composed(hop, k):
        wins = eng.search_sliding_pcm_batch(rec, off, p, WINDOW, hop, k)[0]
        nw = len(wins)
        cut = frames[(np.arange(nw)[:, None] * hop + np.arange(WINDOW)).ravel()]  # one gather, no loop over windows
        ids = np.array([[r["clip_id"] for r in rows] + [-1] * (k - len(rows)) for rows in wins], np.int32)
        al = eng.align_batch(cut, np.arange(nw + 1, dtype=np.int64) * WINDOW, p, ids, k)
        return wins, al

    res = {"workload": f"one {SECONDS} s 8 kHz recording ({nf} frames), window {WINDOW}, vs {args.db_clips} x 30 s clips, "
                       "coefs 1, tolerance 0.001",
           "fused": "tfp_search_sliding_aligned_pcm_batch",
           "composed": "tfp_search_sliding_pcm_batch, the windows cut on the host, tfp_align_batch",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for hop in (1, 8, 47):
        for k in (1, 8):
            before = eng.slide_align_stats()
            f = timed(lambda: eng.search_sliding_aligned_pcm_batch(rec, off, p, WINDOW, hop, k))
            after = eng.slide_align_stats()
            e = timed(lambda: composed(hop, k))
            # the two agree (the PCM form's frames are the recording's own fingerprint)
            got = eng.search_sliding_aligned_pcm_batch(rec, off, p, WINDOW, hop, k)[0]
            wins, al = composed(hop, k)
            keys = ("aligned_count", "offset", "first_frame", "last_frame")
            assert all([[r[x] for x in keys] for r in rows] == [[a[x] for x in keys] for a in al[w][:len(rows)]]
                       for w, rows in enumerate(got))
            res["hop%d_k%d" % (hop, k)] = {
                "windows": len(got), "form": "slid" if after["slid_entries"] > before["slid_entries"] else "direct",
                "fused": f, "composed": e, "fused_to_composed_p50": f["p50_us"] / e["p50_us"]}
    res["slide_align_stats"] = eng.slide_align_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
