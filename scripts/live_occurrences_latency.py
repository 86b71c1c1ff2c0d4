"""Per-tick latency of tfp_live_occurrences against what a caller had before it, at several call ages.

512 channels (--channels), 160-sample ticks, the bench's synthetic DB (bench.enroll: --db-clips x 30 s
clips, default 100,000), coefs = 1, tolerance 0.001, k = 4, every channel playing an excerpt of a DB clip
in scope ANY, a window of about 2 s (--window-ms, 63 frames at 8 kHz): scripts/live_window_aligned_latency.py's
set-up. At each call age (1, 3 and 10 s) three objects are brought to the age by ingest-only pushes and one
untimed call each (so the window tables are current and every track has caught up), and then, per tick and
interleaved in one process after a warm-up, with the order of the three legs rotated from tick to tick, the
script times --reps repetitions of (the tick's ingest-only push is untimed in every leg):
  occurrences: tfp_live_occurrences;
  aligned:     tfp_live_window_aligned alone: the rows and alignments without the log;
  composed:    one tfp_live_frames read-back per channel and one tfp_search_occurrences_batch over the calls
               so far (window, --hop): the log by the calls that existed before, O(recording) per tick.
The claim to check is one of shape: the occurrence call's p50 is flat in the call's age where the
composition's grows; frames_traced per tick is recorded beside it. It records the median, the p99 and the
maximum of each leg per age and writes profiles/live_occurrences_latency.json. Until that file is committed
the figures are unmeasured. Run it under a time limit of its own:

    timeout 1100 python scripts/live_occurrences_latency.py
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


def summary(xs):
    return {"p50": pct(xs, 50), "p99": pct(xs, 99), "max": pct(xs, 100)}


def composed(T, eng, lv, p, k, window, hop, max_gap, min_hits):
    """The log from nch tfp_live_frames + one tfp_search_occurrences_batch over the calls so far."""
    fr = [lv.frames(c, 0) for c in range(lv.nchannels)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])])
    return eng.search_occurrences_batch(np.concatenate(fr), off, p, window, hop, k, max_gap, min_hits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ages", default="1,3,10")
    ap.add_argument("--window-ms", type=int, default=2000)
    ap.add_argument("--hop", type=int, default=8)
    ap.add_argument("--max-gap", type=int, default=8)
    ap.add_argument("--min-hits", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "live_occurrences_latency.json"))
    args = ap.parse_args()
    import torch
    import bench
    import tiresias_amd as T

    dev = torch.device("cuda:0")
    eng = T.Engine(0)
    bench.enroll(eng, torch, dev, 0, list(range(args.db_clips)))
    eng.index_commit()
    ages = [float(a) for a in args.ages.split(",")]
    nch, k = args.channels, 4
    window = T.lib().tfp_live_window_frames(args.window_ms, 8000)
    total = int(max(ages) * 8000) + TICK * (args.reps + args.warmup + 2)
    rng = np.random.default_rng(bench.SEED_Q)
    clips = [int(rng.integers(args.db_clips)) for _ in range(nch)]
    src = T.synth_pcm(bench.SEED_DB, clips, total, offsets=[256 * int(rng.integers(0, 64)) for _ in range(nch)])
    p = T.params(1, 0.001)
    scopes = [-1] * nch
    res = {"workload": f"{nch} channels, {TICK}-sample ticks vs {args.db_clips} x 30 s clips, coefs 1, tolerance 0.001, "
                       f"k {k}, window {window} frames ({args.window_ms} ms), max_gap {args.max_gap}, min_hits {args.min_hits}, "
                       f"composition hop {args.hop}",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "ages": {}}
    legs = ["occurrences", "aligned", "composed"]

    def ask(leg, o):
        if leg == "occurrences":
            return o.occurrences(p, scopes, k, window, args.max_gap, args.min_hits, 64)
        if leg == "aligned":
            return o.window_aligned(p, scopes, k, window)
        return composed(T, eng, o, p, k, window, args.hop, args.max_gap, args.min_hits)

    for age in ages:
        lv = {leg: T.Live(eng, nch, total) for leg in legs}  # a window table each
        s0 = int(age * 8000) // TICK * TICK
        at = 0
        while at < s0:
            n = min(8000, s0 - at)
            for o in lv.values():
                o.push(src[:, at:at + n], None)
            at += n
        for leg in legs:
            ask(leg, lv[leg])
        times = {leg: [] for leg in legs}
        entries, traced0 = 0, None
        for i in range(args.warmup + args.reps):
            blk = src[:, at:at + TICK]
            at += TICK
            for o in lv.values():
                o.push(blk, None)
            if i == args.warmup:
                traced0 = lv["occurrences"].occurrence_stats()["frames_traced"]
            for leg in legs[i % 3:] + legs[:i % 3]:
                t0 = time.perf_counter()
                got = ask(leg, lv[leg])
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times[leg].append(dt)
                if leg == "occurrences":
                    entries += sum(len(ch) for ch in got[0])
        st = lv["occurrences"].occurrence_stats()
        res["ages"]["%g s" % age] = {
            "occurrences_ms": summary(times["occurrences"]),
            "window_aligned_alone_ms": summary(times["aligned"]),
            "frames_occurrences_batch_ms": summary(times["composed"]),
            "entries_per_tick": entries / (args.warmup + args.reps),
            "frames_traced_per_tick": (st["frames_traced"] - traced0) / args.reps,
            "tracks": sum(len(lv["occurrences"].tracks(c)) for c in range(nch)),
            "occurrence_stats": st}
        for o in lv.values():
            o.close()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
