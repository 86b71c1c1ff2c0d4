"""Rate-normalised ingest of int32 Q31 frames: the wide form against the composition a caller had without the
kernel, and the int16 mix form on the same audio as the yardstick for the launch.

The batch is --clips clips (default 1,024) of 5 s of stereo noise at 44100 -> 8000 and at 48000 -> 8000. In
one process, legs interleaved call by call after --warmup calls, p50 / p99 of the wall time over --runs:
  leg 1  Engine.fingerprint_wide_rate_batch (interleaved Q31 host samples in, frames out);
  leg 2  resample_wide_pcm on the host over 16 threads, then Engine.fingerprint_batch of the result;
  leg 3  Engine.fingerprint_mix_rate_batch of the same audio as int16 (the Q31 frames are the int16 frames
         << 16, so legs 1 and 3 give the same frames: half the bytes to the GPU, 4-byte instead of 8-byte sums).
p99 over a few runs is the slowest of them: say the run count beside any figure. Writes
profiles/resample_wide_latency.json. Run under a time limit:

    timeout 700 python scripts/resample_wide_latency.py --runs 8 --warmup 2
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asterisk-tiresias_amd"))

PAIRS = [(44100, 8000), (48000, 8000)]
CHANNELS = 2


def pcts(xs):
    a = np.asarray(xs) * 1e3
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_wide_latency.json"))
    args = ap.parse_args()
    legs = {int(x) for x in args.legs.split(",")}
    import torch
    import tiresias_amd as T

    eng = T.Engine(0)
    pool = ThreadPoolExecutor(16)
    result = {"box": torch.cuda.get_device_name(0), "clips": args.clips, "seconds_per_clip": 5, "channels": CHANNELS,
              "pairs": {}}
    for rin, rout in PAIRS:
        n = 5 * rin  # frames per clip
        pcm = np.random.default_rng(rin).integers(-20000, 20000, (args.clips * n, CHANNELS)).astype(np.int16)
        q31 = pcm.astype(np.int32) << 16
        off = np.arange(args.clips + 1, dtype=np.int64) * n
        n_out = T.resample_count(n, rin, rout)
        ooff = np.arange(args.clips + 1, dtype=np.int64) * n_out
        T.resample_taps(rin, rout)  # the table is built once per process

        def leg1():
            return eng.fingerprint_wide_rate_batch(q31, off, CHANNELS, rin, rout)

        def leg2():
            parts = list(pool.map(lambda c: T.resample_wide_pcm(q31[c * n:(c + 1) * n], CHANNELS, rin, rout),
                                  range(args.clips)))
            return eng.fingerprint_batch(np.concatenate(parts), ooff, rout)

        def leg3():
            return eng.fingerprint_mix_rate_batch(pcm, off, CHANNELS, rin, rout)

        def wall(fn):
            t = time.perf_counter()
            fn()
            return time.perf_counter() - t

        t = {"wide_form": [], "host_then_int16": [], "int16_mix_form": []}
        for i in range(args.warmup + args.runs):
            keep = i >= args.warmup
            for leg, fn, key in ((1, leg1, "wide_form"), (2, leg2, "host_then_int16"), (3, leg3, "int16_mix_form")):
                if leg in legs:
                    v = wall(fn)
                    if keep:
                        t[key].append(v)
        if 1 in legs and 2 in legs:
            a, b = leg1(), leg2()
            assert a.tobytes() == b.tobytes(), "the legs disagree"
        if 1 in legs and 3 in legs:
            assert leg1().tobytes() == leg3().tobytes(), "the wide and the int16 form disagree on widened int16"
        result["pairs"]["%d->%d" % (rin, rout)] = {
            "frames_in": int(len(pcm)), "samples_out": int(args.clips * n_out),
            **{k: pcts(v) for k, v in t.items() if v}}
    result["resample_wide_stats"] = eng.resample_wide_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
