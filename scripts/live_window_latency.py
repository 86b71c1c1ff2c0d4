"""Per-tick latency of tfp_live_window against the two other ways to follow a call, at several call ages.

512 channels (--channels), 160-sample ticks, the bench's synthetic DB (bench.enroll: --db-clips x 30 s
clips, default 100,000), coefs = 1, tolerance 0.001, k = 2, every channel playing an excerpt of a DB clip
in scope ANY, a window of about 2 s (--window-ms, 63 frames at 8 kHz). At each call age (1, 3 and 10 s)
three objects are brought to the age by ingest-only pushes and one untimed searching call each (so the
count tables are current), and then, per tick and interleaved in one process after a warm-up (clocks and
caches), with the order of the three legs rotated from tick to tick, the
script times --reps repetitions of:
  window: an ingest-only tfp_live_push of the tick plus tfp_live_window (the call's last 2 s);
  push:   a searching tfp_live_push of the tick on a second live object (the call so far);
  stream: tfp_stream_push of the tick on a stream whose window is the same 2 s (one winner, no scope;
          it answers nothing until its window is full, so at 1 s it only ingests).
It records the median and p99 of each leg per age with tfp_live_window_stats, checks through
tfp_fingerprint_stats that no window call launched a fingerprint kernel, and writes
profiles/live_window_latency.json. Until that file is committed the figures are unmeasured. Run it under
a time limit of its own:

    timeout 900 python scripts/live_window_latency.py
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
    ap.add_argument("--ages", default="1,3,10")
    ap.add_argument("--window-ms", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "live_window_latency.json"))
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
    window = T.lib().tfp_live_window_frames(args.window_ms, 8000)
    total = int(max(ages) * 8000) + TICK * (args.reps + args.warmup + 2)
    rng = np.random.default_rng(bench.SEED_Q)
    clips = [int(rng.integers(args.db_clips)) for _ in range(nch)]
    src = T.synth_pcm(bench.SEED_DB, clips, total, offsets=[256 * int(rng.integers(0, 64)) for _ in range(nch)])
    p = T.params(1, 0.001)
    scopes = [-1] * nch
    res = {"workload": f"{nch} channels, {TICK}-sample ticks vs {args.db_clips} x 30 s clips, coefs 1, tolerance 0.001, "
                       f"k {k}, window {window} frames ({args.window_ms} ms)",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "ages": {}}
    for age in ages:
        lw, lp = T.Live(eng, nch, total), T.Live(eng, nch, total)
        st = T.Stream(eng, nch, window * 256)
        s0 = int(age * 8000) // TICK * TICK
        at = 0
        while at < s0:  # ingest only, at most a second at a time (a stream tick is at most its window)
            n = min(8000, s0 - at)
            lw.push(src[:, at:at + n], None)
            lp.push(src[:, at:at + n], None)
            st.push(src[:, at:at + n], None)
            at += n
        lw.window(p, scopes, k, window)
        lp.push(src[:, :1], p, scopes, k, nsamples=[0] * nch)
        times = {"window": [], "push": [], "stream": []}
        legs = ["window", "push", "stream"]
        found = 0
        for i in range(args.warmup + args.reps):
            blk = src[:, at:at + TICK]
            at += TICK
            for leg in legs[i % 3:] + legs[:i % 3]:
                if leg == "window":
                    t0 = time.perf_counter()
                    lw.push(blk, None)
                    t1 = time.perf_counter()
                    fp0 = eng.fingerprint_stats()  # (untimed)
                    t2 = time.perf_counter()
                    lw.window(p, scopes, k, window)
                    t3 = time.perf_counter()
                    assert eng.fingerprint_stats() == fp0, "a window call launched a fingerprint kernel"
                    dt = (t1 - t0) + (t3 - t2)
                elif leg == "push":
                    t0 = time.perf_counter()
                    lp.push(blk, p, scopes, k)
                    dt = time.perf_counter() - t0
                else:
                    t0 = time.perf_counter()
                    r = st.push(blk, p)
                    dt = time.perf_counter() - t0
                    found += sum(x is not None for x in r)
                if i >= args.warmup:
                    times[leg].append(dt)
        res["ages"]["%g s" % age] = {
            "push_ingest_plus_window_ms": {"p50": pct(times["window"], 50), "p99": pct(times["window"], 99)},
            "searching_push_ms": {"p50": pct(times["push"], 50), "p99": pct(times["push"], 99)},
            "stream_push_ms": {"p50": pct(times["stream"], 50), "p99": pct(times["stream"], 99)},
            "stream_found_per_tick": found / (args.warmup + args.reps),
            "window_stats": lw.window_stats(), "live_stats_of_the_searching_push": lp.stats()}
        lw.close()
        lp.close()
        st.close()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
