"""Per-tick latency of tfp_live_window_aligned against what a caller had before it, at several call ages.

512 channels (--channels), 160-sample ticks, the bench's synthetic DB (bench.enroll: --db-clips x 30 s
clips, default 100,000), coefs = 1, tolerance 0.001, k = 4, every channel playing an excerpt of a DB clip
in scope ANY, a window of about 2 s (--window-ms, 63 frames at 8 kHz). At each call age (1, 3 and 10 s)
three objects are brought to the age by ingest-only pushes and one untimed call each (so the window
tables are current), and then, per tick and interleaved in one process after a warm-up, with the order of
the three legs rotated from tick to tick, the script times --reps repetitions of (the tick's ingest-only
push is untimed in every leg: it is the same in all three):
  aligned:  tfp_live_window_aligned;
  window:   (a) tfp_live_window alone: the rows without the alignments;
  composed: (b) tfp_live_window, one tfp_live_frames read-back per channel, and one tfp_align_batch over
            the windows and the rows' clips: the same answer by the calls that existed before.
The aligned and the composed answers are compared on every tick. It records the median, the p99 (200
repetitions by default, so that it is a percentile and not the worst call) and the maximum of each
leg per age and writes profiles/live_window_aligned_latency.json. Until that file is committed the
figures are unmeasured. Run it under a time limit of its own:

    timeout 900 python scripts/live_window_aligned_latency.py
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


def composed(T, eng, lv, p, scopes, k, window):
    """The rows and alignments from tfp_live_window + nch tfp_live_frames + one tfp_align_batch."""
    rows, fc, ff = lv.window(p, scopes, k, window)
    nch = lv.nchannels
    fr = [lv.frames(c, ff[c]) for c in range(nch)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])])
    ids = np.full(nch * k, -1, np.int32)
    for c in range(nch):
        got = [r["clip_id"] for r in rows[c]]
        ids[c * k:c * k + len(got)] = got
    al = eng.align_batch(np.concatenate(fr) if off[-1] else np.zeros(1, T.FRAME_DTYPE), off, p, ids, k)
    return rows, al, fc, ff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ages", default="1,3,10")
    ap.add_argument("--window-ms", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "live_window_aligned_latency.json"))
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
                       f"k {k}, window {window} frames ({args.window_ms} ms)",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "ages": {}}
    legs = ["aligned", "window", "composed"]
    for age in ages:
        lv = {leg: T.Live(eng, nch, total) for leg in legs}  # a window table each
        s0 = int(age * 8000) // TICK * TICK
        at = 0
        while at < s0:
            n = min(8000, s0 - at)
            for o in lv.values():
                o.push(src[:, at:at + n], None)
            at += n
        lv["aligned"].window_aligned(p, scopes, k, window)
        lv["window"].window(p, scopes, k, window)
        composed(T, eng, lv["composed"], p, scopes, k, window)
        times = {leg: [] for leg in legs}
        rows_per_tick = 0
        for i in range(args.warmup + args.reps):
            blk = src[:, at:at + TICK]
            at += TICK
            for o in lv.values():
                o.push(blk, None)
            got = {}
            for leg in legs[i % 3:] + legs[:i % 3]:
                t0 = time.perf_counter()
                if leg == "aligned":
                    got[leg] = lv[leg].window_aligned(p, scopes, k, window)
                elif leg == "window":
                    got[leg] = lv[leg].window(p, scopes, k, window)
                else:
                    got[leg] = composed(T, eng, lv[leg], p, scopes, k, window)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times[leg].append(dt)
            rows, al, fc, ff = got["aligned"]
            assert (rows, fc, ff) == got["window"], "the aligned call's rows are not tfp_live_window's"
            assert (rows, al, fc, ff) == got["composed"], "the aligned call's alignments are not tfp_align_batch's"
            rows_per_tick += sum(len(r) for r in rows)
        res["ages"]["%g s" % age] = {
            "window_aligned_ms": summary(times["aligned"]),
            "window_alone_ms": summary(times["window"]),
            "window_frames_align_batch_ms": summary(times["composed"]),
            "rows_per_tick": rows_per_tick / (args.warmup + args.reps),
            "window_aligned_stats": lv["aligned"].window_aligned_stats(), "window_stats": lv["aligned"].window_stats()}
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
