"""Per-tick latency of tfp_live_push against the only other way to get the same rows, at several call ages.

512 channels (--channels), 160-sample ticks, the bench's synthetic DB (bench.enroll: --db-clips x 30 s
clips, default 100,000), coefs = 1, tolerance 0.001, k = 2, every channel playing an excerpt of a DB clip
in scope ANY. At each call age (0.5, 1, 3 and 10 s) the script times, interleaved in one process after a
warm-up (clocks and caches), --reps repetitions of: one tfp_live_push tick at that
age (the calls are brought to the age by ingest-only pushes and one untimed searching push, so the
count table is current), and one tfp_search_scoped_pcm_batch over the 512 prefixes of that age (unchanged
code: what a caller must do today), and the record loop's own form on a second live object fed the same
calls as mu-law payload: one ingest-only tfp_live_push_g711 tick and one tfp_live_verdict. It records
p50 / p99 of each leg and the prefix / live ratio per age, checks that the rows agree, and writes
profiles/live_latency.json. It has not been run: no latency of a live call is measured yet. Run it
under a time limit of its own:

    timeout 900 python scripts/live_latency.py
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

TICK = 160


def pct(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e3, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ages", default="0.5,1,3,10")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "live_latency.json"))
    args = ap.parse_args()
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    ages = [float(a) for a in args.ages.split(",")]
    nch, k = args.channels, 2
    total = int(max(ages) * 8000) + TICK * (args.reps + args.warmup + 2)
    rng = np.random.default_rng(bench.SEED_Q)
    clips = [int(rng.integers(args.db_clips)) for _ in range(nch)]
    src = T.synth_pcm(bench.SEED_DB, clips, total, offsets=[256 * int(rng.integers(0, 64)) for _ in range(nch)])
    p = T.params(1, 0.001)
    scopes = [-1] * nch
    # the same calls as mu-law payload (the nearest code per sample), planned to last `total` samples
    table = T.decode_g711(np.arange(256, dtype=np.uint8), T.ULAW).astype(np.int32)
    order = np.argsort(table, kind="stable")
    codes = order[np.clip(np.searchsorted(table[order], src.astype(np.int32)), 0, 255)].astype(np.uint8)
    totals = [total] * nch
    res = {"workload": f"{nch} channels, {TICK}-sample ticks vs {args.db_clips} x 30 s clips, coefs 1, tolerance 0.001, k {k}",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "ages": {}}
    for age in ages:
        lv = T.Live(eng, nch, total)
        s0 = int(age * 8000) // TICK * TICK
        at = 0
        while at + 8000 <= s0:  # ingest only, a second at a time
            lv.push(src[:, at:at + 8000], None)
            at += 8000
        if at < s0:
            lv.push(src[:, at:s0], None)
        lg = T.Live(eng, nch, total)
        if s0:
            lg.push_g711(codes[:, :s0], T.ULAW, None)
        at = s0
        live_t, pre_t, g711_t, verdict_t, decided = [], [], [], [], 0
        for i in range(args.warmup + args.reps):
            blk = src[:, at:at + TICK]
            t0 = time.perf_counter()
            rows, _ = lv.push(blk, p, scopes, k)
            t1 = time.perf_counter()
            at += TICK
            off = np.arange(nch + 1, dtype=np.int64) * at
            pre = np.ascontiguousarray(src[:, :at]).reshape(-1)
            t2 = time.perf_counter()
            want = eng.search_scoped_pcm_batch(pre, off, p, scopes, k)
            t3 = time.perf_counter()
            assert rows == want, (age, i)
            # the record loop's form: the tick as G.711 payload, ingest only, then the verdict (on a second
            # object fed the same call as mu-law codes, so the int16 leg above stays what it was)
            t4 = time.perf_counter()
            lg.push_g711(codes[:, at - TICK:at], T.ULAW, None)
            t5 = time.perf_counter()
            v = lg.verdict(totals, p, scopes)
            t6 = time.perf_counter()
            decided += sum(x["decided"] for x in v)
            if i >= args.warmup:
                live_t.append(t1 - t0)
                pre_t.append(t3 - t2)
                g711_t.append(t5 - t4)
                verdict_t.append(t6 - t5)
        st = lv.stats()
        lv.close()
        lg.close()
        res["ages"]["%g s" % age] = {
            "live_push_ms": {"p50": pct(live_t, 50), "p99": pct(live_t, 99)},
            "g711_ingest_push_ms": {"p50": pct(g711_t, 50), "p99": pct(g711_t, 99)},
            "verdict_ms": {"p50": pct(verdict_t, 50), "p99": pct(verdict_t, 99)},
            "decided_per_verdict": decided / (nch * (args.warmup + args.reps)),
            "prefix_search_ms": {"p50": pct(pre_t, 50), "p99": pct(pre_t, 99)},
            "prefix_over_live_p50": pct(pre_t, 50) / pct(live_t, 50), "live_stats": st}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
