"""The calls' aligned trailing windows at the module's facade: fp_live_window_aligned of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_live_window_aligned_harness.c) over a group of
three engines on device 0 ("0,0,0"). Its JSON equals fp_live_window's plus, per row, aligned_count, offset,
first_frame, last_frame and clip_start_frame = the channel's first_frame - offset; the five equal
Live.window_aligned of the ctypes mirror on an engine that holds the same prompts and took the same
samples. NULL for window_ms <= 0 and k < 1 (checked by the harness)."""
import json
import os
import subprocess

import numpy as np
import pytest

import verdict_util as V
from conftest import REPO
from g711_util import ULAW, encode, expand

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
PROMPTS = {"a": (V.ZLEAD, 6), "b": (V.LONE, 7)}
K = 3
ASKS = [(10, 32, 1), (10, 224, 7), (19, 65, 3), (20, 2000, 63), (20, 224, 7)]  # (tick, window_ms, frames)
FIVE = ("aligned_count", "offset", "first_frame", "last_frame", "clip_start_frame")


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_live_window_aligned")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC,
                    os.path.join(NATIVE, "shim_live_window_aligned_harness.c"), stubs, str(tmp_path / "fp_handler_tfp.c.o"),
                    str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib, "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS],
                   check=True)
    return exe


def test_shim_live_window_aligned(tmp_path, tfp_lib, engine):
    from tiresias_amd.fp_handler import write_wav_mono16
    exe = _build(tmp_path, os.path.dirname(tfp_lib.LIB_PATH))
    files, clips = [], []
    for ctx in ("a", "b"):
        for c in PROMPTS[ctx]:
            files.append(str(tmp_path / ("%s_clip%d.wav" % (ctx, c))))
            write_wav_mono16(files[-1], V.clip_pcm(c))
            clips.append((ctx, c))
    calls = [np.concatenate([V.clip_pcm(6)[512:512 + 1920], V.clip_pcm(V.ZLEAD)[256:256 + 1280]]), V.clip_pcm(V.LONE)[256:256 + 3000]]
    heard = []
    for ch, x in enumerate(calls):
        codes = encode(x, ULAW)
        heard.append(expand(codes, ULAW).astype(np.int16))
        (tmp_path / ("ch%d.ulaw" % ch)).write_bytes(codes.tobytes())
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), str(V.TOL), str(K), str(tmp_path / "ch0.ulaw"),
                        str(tmp_path / "ch1.ulaw"), *files, *["%d:%d" % (t, ms) for t, ms, _ in ASKS]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout.splitlines()[-1])
    uuid = {os.path.basename(e["name"]): e["uuid"] for ctx in ("a", "b") for e in out["catalog"][ctx]}
    engine.index_clear()
    try:
        for f, (ctx, c) in zip(files, clips):
            fr = engine.fingerprint(V.clip_pcm(c))
            engine.index_add(uuid[os.path.basename(f)], fr["m1"], fr["m2"])
        engine.index_set_scope([uuid[os.path.basename(f)] for f in files], [0, 0, 1, 1])
        lv = tfp_lib.Live(engine, 2, 16000)
        p = tfp_lib.params(1, V.TOL)
        assert [(a["tick"], a["window_ms"]) for a in out["asks"]] == [(t, ms) for t, ms, _ in ASKS]
        tick, some_rows = 0, 0
        for got, (at, ms, frames) in zip(out["asks"], ASKS):
            while tick < at:
                n = [max(0, min(160, len(h) - tick * 160)) for h in heard]
                blk = np.zeros((2, 160), np.int16)
                for c in range(2):
                    blk[c, :n[c]] = heard[c][tick * 160:tick * 160 + n[c]]
                lv.push(blk, None, nsamples=n)
                tick += 1
            rows, al, fc, ff = lv.window_aligned(p, [0, 1], K, frames)
            for c in range(2):
                plain, ali = got["plain"][c], got["aligned"][c]
                # fp_live_window's JSON plus the five fields
                assert {k: v for k, v in ali.items() if k != "rows"} == {k: v for k, v in plain.items() if k != "rows"}
                assert [{k: v for k, v in x.items() if k not in FIVE} for x in ali["rows"]] == plain["rows"], (at, ms, c)
                assert (ali["first_frame"], ali["frame_count"]) == (ff[c], fc[c])
                assert [x["uuid"] for x in ali["rows"]] == [x["audio_uuid"] for x in rows[c]], (at, ms, c)
                for x, a in zip(ali["rows"], al[c]):
                    assert {f: x[f] for f in FIVE[:4]} == a, (at, ms, c)
                    assert x["clip_start_frame"] == ali["first_frame"] - x["offset"]
                some_rows += len(ali["rows"])
        assert some_rows
        lv.close()
    finally:
        engine.index_clear()
