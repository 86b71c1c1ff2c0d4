"""Mixed batches: one fingerprint_any_batch against the per-class calls the mirror makes without it.

The batch is --clips clips (default 1,024) of 5 s of noise into a 16000 Hz index, split evenly over four
classes: int16 mono at 16000 (the index rate: no filter), int16 stereo at 44100, int32 Q31 stereo at 48000 and
mu-law at 8000. In one process, legs interleaved call by call after --warmup calls, p50 / p99 of the wall time
over --runs:
  leg 1  Engine.fingerprint_any_batch of the whole batch (the bytes as they are in, frames out; one conversion
         launch);
  leg 2  the four calls of today's directory enrolment: fingerprint_batch, fingerprint_mix_rate_batch,
         fingerprint_wide_rate_batch, and decode_g711 on the host followed by fingerprint_rate_batch.
Both legs give the same frames (checked once). p99 over a few runs is the slowest of them: say the run count
beside any figure. Whole calls only: the conversion launch alone is not traced. Writes
profiles/resample_any_latency.json. Run under a time limit:

    timeout 700 python scripts/resample_any_latency.py --runs 8 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asterisk-tiresias_amd"))

RATE_OUT = 16000


def pcts(xs):
    a = np.asarray(xs) * 1e3
    return {"p50_ms": float(np.percentile(a, 50)), "p99_ms": float(np.percentile(a, 99)), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_any_latency.json"))
    args = ap.parse_args()
    import torch
    import tiresias_amd as T

    eng = T.Engine(0)
    per = args.clips // 4
    rng = np.random.default_rng(5)
    mono = rng.integers(-20000, 20000, per * 5 * 16000).astype(np.int16)
    stereo = rng.integers(-20000, 20000, (per * 5 * 44100, 2)).astype(np.int16)
    q31 = rng.integers(-2**30, 2**30, (per * 5 * 48000, 2)).astype(np.int32)
    ulaw = rng.integers(0, 256, per * 5 * 8000).astype(np.uint8)
    off = {r: np.arange(per + 1, dtype=np.int64) * 5 * r for r in (16000, 44100, 48000, 8000)}
    # the mixed call's bytes: the four arrays end to end (each a multiple of 4 bytes long), one descriptor per clip
    parts = [(mono, 16000, 1, T.AUDIO_S16, 2), (stereo, 44100, 2, T.AUDIO_S16, 2), (q31, 48000, 2, T.AUDIO_Q31, 4),
             (ulaw, 8000, 1, T.AUDIO_ULAW, 1)]
    data = np.concatenate([np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x, *_ in parts])
    clips = np.zeros(4 * per, T.CLIP_DTYPE)
    pos = 0
    for k, (x, rate, ch, kind, ss) in enumerate(parts):
        assert pos % 4 == 0
        c = clips[k * per:(k + 1) * per]
        c["offset"] = pos + np.arange(per, dtype=np.int64) * 5 * rate * ch * ss
        c["nframes"], c["rate_in"], c["channels"], c["kind"] = 5 * rate, rate, ch, kind
        pos += x.nbytes
    for r in (44100, 48000, 8000):
        T.resample_taps(r, RATE_OUT)  # the tables are built once per process

    def leg1():
        return eng.fingerprint_any_batch(data, clips, RATE_OUT)

    def leg2():
        return np.concatenate([
            eng.fingerprint_batch(mono, off[16000], RATE_OUT),
            eng.fingerprint_mix_rate_batch(stereo, off[44100], 2, 44100, RATE_OUT),
            eng.fingerprint_wide_rate_batch(q31, off[48000], 2, 48000, RATE_OUT),
            eng.fingerprint_rate_batch(T.decode_g711(ulaw, T.ULAW), off[8000], 8000, RATE_OUT)])

    def wall(fn):
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t

    t = {"any_batch": [], "per_class_calls": []}
    for i in range(args.warmup + args.runs):
        for fn, key in ((leg1, "any_batch"), (leg2, "per_class_calls")):
            v = wall(fn)
            if i >= args.warmup:
                t[key].append(v)
    assert leg1().tobytes() == leg2().tobytes(), "the legs disagree"
    result = {"box": torch.cuda.get_device_name(0), "clips": 4 * per, "seconds_per_clip": 5, "rate_out": RATE_OUT,
              "classes": ["s16 mono 16000", "s16 stereo 44100", "q31 stereo 48000", "ulaw 8000"], "bytes_in": int(len(data)),
              **{k: pcts(v) for k, v in t.items()}, "resample_any_stats": eng.resample_any_stats()}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
