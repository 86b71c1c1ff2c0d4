"""Latency of tfp_index_neighbours against what a caller had before it.

The bench's synthetic DB (bench.enroll: --db-clips x 30 s clips, default 100,000), coefs = 1, tolerance
0.001, k = 4, scope ANY. For 1, 64 and 512 named clips (seeded picks), interleaved in one process after a
warm-up with the order of the two legs alternating, the script times --reps repetitions (at least 30) of
  neighbours: one tfp_index_neighbours call with alignments;
  composed:   tfp_index_rows per clip, frames built on the host, tfp_search_scoped_batch at k + 1 with the
              clip itself removed, tfp_align_batch on the remaining rows.
It checks once per size that both legs return the same rows and alignments, records the median, the p99 and
the maximum of each leg and writes profiles/neighbours_latency.json. Until that file is committed the
figures are unmeasured. Run it under a time limit of its own:

    timeout 1100 python scripts/neighbours_latency.py
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

NULL = -(2**31)
FOUR = ("aligned_count", "offset", "first_frame", "last_frame")


def pct(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e3, p))


def summary(xs):
    return {"p50": pct(xs, 50), "p99": pct(xs, 99), "max": pct(xs, 100)}


def composed(T, eng, uuids, p, k):
    """Per clip (rows as (uuid, count), alignments) by the calls that existed before."""
    frames = []
    for u in uuids:
        m1, m2 = eng.index_rows(u)
        fr = np.zeros(len(m1), T.FRAME_DTYPE)
        fr["q1"] = np.where(m1 == NULL, -np.inf, m1 / 1e6)
        fr["q2"] = np.where(m2 == NULL, -np.inf, m2 / 1e6)
        frames.append(fr)
    fr = np.concatenate(frames)
    qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    found = eng.search_scoped_batch(fr, qoff, p, [-1] * len(uuids), k + 1)
    rows = [[r for r in found[i] if r["audio_uuid"] != uuids[i]][:k] for i in range(len(uuids))]
    ids = np.asarray([[r["clip_id"] for r in rs] + [-1] * (k - len(rs)) for rs in rows], np.int32).reshape(-1)
    al = eng.align_batch(fr, qoff, p, ids, k)
    return [([(r["audio_uuid"], r["match_count"]) for r in rows[i]], [tuple(a[f] for f in FOUR) for a in al[i][:len(rows[i])]])
            for i in range(len(uuids))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--sizes", default="1,64,512")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neighbours_latency.json"))
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps below 30")
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    p, k = T.params(1, 0.001), 4
    rng = np.random.default_rng(bench.SEED_Q)
    res = {"workload": f"{args.db_clips} x 30 s clips, coefs 1, tolerance 0.001, k {k}, scope ANY, with alignments",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "named": {}}
    for n in [int(x) for x in args.sizes.split(",")]:
        uuids = [bench.uuid_of(int(g)) for g in rng.choice(args.db_clips, n, replace=False)]
        legs = {"neighbours": lambda: eng.index_neighbours(uuids, p, k), "composed": lambda: composed(T, eng, uuids, p, k)}
        a, b = legs["neighbours"](), legs["composed"]()
        same = [([(r["audio_uuid"], r["match_count"]) for r in x["neighbours"]], [tuple(r[f] for f in FOUR) for r in x["neighbours"]])
                for x in a] == b
        before = eng.neighbour_stats()
        times = {leg: [] for leg in legs}
        order = list(legs)
        for i in range(args.warmup + args.reps):
            for leg in order[i % 2:] + order[:i % 2]:
                t0 = time.perf_counter()
                legs[leg]()
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times[leg].append(dt)
        after = eng.neighbour_stats()
        res["named"][str(n)] = {"neighbours_ms": summary(times["neighbours"]), "rows_scoped_align_ms": summary(times["composed"]),
                                "legs_agree": bool(same), "rows": sum(len(x["neighbours"]) for x in a),
                                "vote_calls": after["vote_batches"] - before["vote_batches"],
                                "general_calls": after["general_batches"] - before["general_batches"]}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
