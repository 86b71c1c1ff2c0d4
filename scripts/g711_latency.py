"""Latency of the G.711 code forms against the path a caller had before them, for the same audio:
a host table expansion (numpy take over the 256-entry table) followed by the int16 call.

Three measurements, each arm's repetitions interleaved (A B A B ...), --reps repetitions, medians
and the spread (min .. max) over the repetitions; nothing is gated on them:

  (a) stream tick at configs[4] (512 channels x 160 samples, 3 s window, matched every tick against
      --db-clips enrolled clips): p50 / p99 per tick through Stream.push_g711 and through the table
      take + Stream.push, two streams fed the same audio in alternating blocks of ticks;
  (b) host-batch enrolment of --enrol-clips x 30 s clips: wall time of one fingerprint_g711_batch
      against the table take + fingerprint_batch (expansion counted on the baseline's side);
  (c) batch-1 search of a 5 s query from Python: p50 of search_g711_batch against the table take +
      search_pcm_batch; both copy the query into the engine's mapped staging, the code form half
      the bytes plus one small launch. A third arm is the zero-copy int16 path: the query already
      expanded in a tfp_host_alloc buffer (no take, no copy), which the GPU reads in place. Against
      that arm the code form pays its copy and its extra launch; the difference is reported.

Writes profiles/g711_latency.json and prints it. Run it under a time limit of its own:

    timeout 900 python scripts/g711_latency.py
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "asterisk-tiresias_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

SEED_DB = 0x7153A1


def us(xs, p):
    return float(np.percentile(np.asarray(xs) * 1e6, p))


def spread(vals):
    return {"median": float(np.median(vals)), "min": float(np.min(vals)), "max": float(np.max(vals))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-clips", type=int, default=2000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--enrol-clips", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "g711_latency.json"))
    args = ap.parse_args()
    import tiresias_amd as T
    from g711_util import ULAW, encode, expand

    law = ULAW
    table = expand(np.arange(256, dtype=np.uint8), law)
    eng = T.Engine(0)
    n_db = 8000 * 10
    for a in range(0, args.db_clips, 250):  # the index the ticks and the queries are matched against
        ids = list(range(a, min(a + 250, args.db_clips)))
        fr = eng.fingerprint_batch(T.synth_pcm(SEED_DB, ids, n_db).reshape(-1), np.arange(len(ids) + 1) * n_db)
        nf = len(fr) // len(ids)
        eng.index_add_batch(["%08x-7110-4000-8000-%012x" % (c * 2654435761 % 2**32, c) for c in ids],
                            np.arange(len(ids) + 1) * nf, fr["m1"], fr["m2"])
    eng.index_commit()
    p = T.params(1, 0.001)
    out = {"law": "ulaw", "reps": args.reps, "db_clips": args.db_clips,
           "baseline": "numpy take over the 256-entry table, then the int16 call (the parent commit's path)"}

    # (a) stream ticks
    nch, W, tick = args.channels, 24000, 160
    span = 64000  # per channel; played round and round (a seam every 8 s does not change a tick's cost)
    src = encode(T.synth_pcm(SEED_DB, [c % args.db_clips for c in range(nch)], span, offsets=[256 * c for c in range(nch)]), law)
    sa, sb = T.Stream(eng, nch, W), T.Stream(eng, nch, W)
    pos = 0

    def block(st, code_form, n, timed):
        nonlocal pos
        ts = []
        for _ in range(n):
            codes = np.ascontiguousarray(src[:, pos:pos + tick])
            pos = pos + tick if pos + 2 * tick <= span else 0
            t0 = time.perf_counter()
            if code_form:
                st.push_g711(codes, law, p)
            else:
                st.push(table[codes], p)
            ts.append(time.perf_counter() - t0)
        return ts if timed else []

    for t in range(W // tick):  # fill both windows (ingest only), same audio
        codes = np.ascontiguousarray(src[:, pos:pos + tick])
        pos = pos + tick if pos + 2 * tick <= span else 0
        sa.push_g711(codes, law)
        sb.push(table[codes])
    block(sa, True, 20, False), block(sb, False, 20, False)
    rows = {"g711": [], "table_take_int16": []}
    for _ in range(args.reps):
        a = block(sa, True, args.ticks, True)
        b = block(sb, False, args.ticks, True)
        rows["g711"].append((us(a, 50), us(a, 99)))
        rows["table_take_int16"].append((us(b, 50), us(b, 99)))
    out["stream_tick_us"] = {"channels": nch, "tick_samples": tick, "window_samples": W, "ticks_per_rep": args.ticks,
                             **{k: {"p50": spread([r[0] for r in v]), "p99": spread([r[1] for r in v])}
                                for k, v in rows.items()}}
    sa.close(), sb.close()

    # (b) host-batch enrolment
    n30 = 8000 * 30
    chunk = encode(T.synth_pcm(SEED_DB, range(64), n30), law).reshape(-1)
    codes = np.tile(chunk, args.enrol_clips // 64)
    off = np.arange(args.enrol_clips + 1, dtype=np.int64) * n30
    eng.fingerprint_g711_batch(codes, off, law)  # warm both arms' buffers
    eng.fingerprint_batch(table[codes], off)
    ta, tb = [], []
    for r in range(args.reps):
        codes = np.roll(codes, 4001 * (r + 1))  # other audio every repetition: no result can be a leftover
        pcm = table[codes]
        del pcm  # (the pages stay warm; the timed take below allocates its own result)
        t0 = time.perf_counter()
        fa = eng.fingerprint_g711_batch(codes, off, law)
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        fb = eng.fingerprint_batch(table[codes], off)
        tb.append(time.perf_counter() - t0)
        assert np.array_equal(fa["m1"], fb["m1"]) and np.array_equal(fa["m2"], fb["m2"])
    out["enrol_batch_s"] = {"clips": args.enrol_clips, "seconds_per_clip": 30, "g711": spread(ta),
                            "table_take_int16": spread(tb)}
    del codes

    # (c) batch-1 search, 5 s query
    q = np.ascontiguousarray(encode(T.synth_pcm(SEED_DB, [17], 40000, offsets=[256 * 40])[0], law))
    qo = np.array([0, len(q)], np.int64)
    for _ in range(30):
        eng.search_g711_batch(q, qo, law, p), eng.search_pcm_batch(table[q], qo, p)
    hp = ctypes.c_void_p()
    T._lib.check(T.lib().tfp_host_alloc(2 * len(q), ctypes.byref(hp)))
    qz = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_int16)), (len(q),))
    qz[:] = table[q]
    for _ in range(30):
        eng.search_pcm_batch(qz, qo, p)
    ra, rb, rc = [], [], []
    for _ in range(args.reps):
        a, b, c = [], [], []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            r1 = eng.search_g711_batch(q, qo, law, p)
            a.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r2 = eng.search_pcm_batch(table[q], qo, p)
            b.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r3 = eng.search_pcm_batch(qz, qo, p)
            c.append(time.perf_counter() - t0)
        assert r1 == r2 == r3
        ra.append(us(a, 50)), rb.append(us(b, 50)), rc.append(us(c, 50))
    out["search_batch1_p50_us"] = {"query_samples": len(q), "calls_per_rep": args.calls, "g711": spread(ra),
                                   "table_take_int16": spread(rb), "zero_copy_int16": spread(rc),
                                   "difference_of_medians": float(np.median(ra) - np.median(rb)),
                                   "g711_minus_zero_copy_int16": float(np.median(ra) - np.median(rc))}
    del qz
    T.lib().tfp_host_free(hp)
    out["g711_stats"] = eng.g711_stats()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
