"""Rate-normalised ingest: the rate form against the composition a caller has without the kernel, and the
resample launch beside two yardsticks.

The batch is --clips clips (default 1,024) of 5 s of noise at 44100 -> 8000 and at 16000 -> 8000. In one
process, legs interleaved call by call after --warmup calls, p50 / p99 over --runs:
  leg 1  Engine.fingerprint_rate_batch (host samples in, frames out);
  leg 2  resample_pcm on the host over 16 threads, then Engine.fingerprint_batch of the result;
  leg 3  yardsticks timed with device events: a device-to-device copy of the input bytes, and the fingerprint
         launch of the output (tfp_fingerprint_device on a plan of the output lengths).
The resample launch alone has no entry point of its own, so it is timed in two steps: a kernel trace of
leg 1 run on its own, then the run that writes the file and folds the trace in (resample_launch_ms: the
traced launches per pair, in call order; resample_kernel_trace: the trace's own statistics). p99 over
a few runs is the slowest of them: say the run count beside any figure. profiles/resample_latency.json
was written with, each step under a time limit of its own:

    timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rsprof -o rs -- \
        python scripts/resample_latency.py --legs 1 --runs 3 --warmup 1 --out /tmp/leg1.json
    timeout 700 python scripts/resample_latency.py --runs 8 --warmup 2 \
        --kernel-stats /tmp/rsprof/rs_kernel_stats.csv --kernel-trace /tmp/rsprof/rs_kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asterisk-tiresias_amd"))

PAIRS = [(44100, 8000), (16000, 8000)]


def pcts(xs):
    a = np.asarray(xs) * 1e3
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel_stats.csv of a --legs 1 run")
    ap.add_argument("--kernel-trace", default=None, help="rocprofv3's kernel_trace.csv of the same run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_latency.json"))
    args = ap.parse_args()
    legs = {int(x) for x in args.legs.split(",")}
    import torch
    import tiresias_amd as T

    eng = T.Engine(0)
    pool = ThreadPoolExecutor(16)
    result = {"box": torch.cuda.get_device_name(0), "clips": args.clips, "seconds_per_clip": 5, "pairs": {}}
    for rin, rout in PAIRS:
        n = 5 * rin
        pcm = np.random.default_rng(rin).integers(-20000, 20000, args.clips * n).astype(np.int16)
        off = np.arange(args.clips + 1, dtype=np.int64) * n
        n_out = T.resample_count(n, rin, rout)
        ooff = np.arange(args.clips + 1, dtype=np.int64) * n_out
        T.resample_taps(rin, rout)  # the table is built once per process

        def leg1():
            return eng.fingerprint_rate_batch(pcm, off, rin, rout)

        def leg2():
            parts = list(pool.map(lambda c: T.resample_pcm(pcm[c * n:(c + 1) * n], rin, rout), range(args.clips)))
            return eng.fingerprint_batch(np.concatenate(parts), ooff, rout)

        d_in = torch.from_numpy(pcm).cuda()
        d_copy = torch.empty_like(d_in)
        plan = T.Plan(eng, ooff, rout)
        d_out = torch.zeros(args.clips * n_out, dtype=torch.int16, device="cuda")
        d_micro = torch.zeros(2 * plan.nframes + 2, dtype=torch.int32, device="cuda")

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        def wall(fn):
            t = time.perf_counter()
            fn()
            return time.perf_counter() - t

        t = {"rate_form": [], "host_then_int16": [], "d2d_copy": [], "fingerprint_launch": []}
        for i in range(args.warmup + args.runs):
            keep = i >= args.warmup
            if 1 in legs:
                v = wall(leg1)
                if keep:
                    t["rate_form"].append(v)
            if 2 in legs:
                v = wall(leg2)
                if keep:
                    t["host_then_int16"].append(v)
            if 3 in legs:
                v = timed(lambda: d_copy.copy_(d_in))
                w = timed(lambda: eng.fingerprint_device(plan, d_out.data_ptr(), d_micro.data_ptr()))
                if keep:
                    t["d2d_copy"].append(v)
                    t["fingerprint_launch"].append(w)
        if 1 in legs and 2 in legs:
            a, b = leg1(), leg2()
            assert a.tobytes() == b.tobytes(), "the legs disagree"
        result["pairs"]["%d->%d" % (rin, rout)] = {
            "samples_in": int(len(pcm)), "samples_out": int(args.clips * n_out),
            **{k: pcts(v) for k, v in t.items() if v}}
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "resample_kernel" in r.get("Name", "")]
        result["resample_kernel_trace"] = [{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in r}
                                           for r in rows]
    if args.kernel_trace:
        with open(args.kernel_trace) as f:
            ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in csv.DictReader(f)
                  if "resample_kernel" in r["Kernel_Name"]]
        per = len(ms) // len(PAIRS)  # the traced run made the same calls for every pair, pair after pair
        result["resample_launch_ms"] = {"%d->%d" % pr: ms[i * per:(i + 1) * per] for i, pr in enumerate(PAIRS)}
        result["resample_launch_ms"]["from"] = "a kernel trace of a run of leg 1 alone, launches in call order"
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
