"""The calls' trailing windows at the module's facade: fp_live_window of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_live_window_harness.c) over a group of three
engines on device 0 ("0,0,0"). 4 prompts in two contexts, two channels pushed as mu-law payload (one
with a short last tick): the JSON of every ask equals Live.window of the ctypes mirror on an engine that
holds the same prompts and took the same samples, each row carries its catalog fields, and window_ms
becomes ceil(window_ms * rate / 1000 / 256) frames, at least 1 (application_handler.c:152-185, :248-312)."""
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
# (tick, window_ms, frames): 32 ms is exactly one frame of 256 samples at 8 kHz, 33 ms needs a second;
# 224 ms is exactly 7, 225 ms needs an 8th; 1 ms is still a frame; 2,000 ms is longer than the calls
ASKS = [(10, 32, 1), (10, 33, 2), (10, 224, 7), (10, 225, 8), (19, 1, 1), (19, 64, 2), (19, 65, 3), (20, 2000, 63), (20, 224, 7)]


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_live_window")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_live_window_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    return exe


def test_shim_live_window(tmp_path, tfp_lib, engine):
    from tiresias_amd.fp_handler import write_wav_mono16
    for ms, frames in {(ms, fr) for _, ms, fr in ASKS}:
        assert tfp_lib.lib().tfp_live_window_frames(ms, 8000) == frames == max(1, -(-ms * 8000 // 256000))
    exe = _build(tmp_path, os.path.dirname(tfp_lib.LIB_PATH))
    files, clips = [], []
    for ctx in ("a", "b"):
        for c in PROMPTS[ctx]:
            files.append(str(tmp_path / ("%s_clip%d.wav" % (ctx, c))))
            write_wav_mono16(files[-1], V.clip_pcm(c))
            clips.append((ctx, c))
    # channel 0 leaves its context's second prompt for its first after 7.5 frames; channel 1's last tick is short
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
    uuid, ctx_of = {}, {}
    for ctx in ("a", "b"):
        assert len(out["catalog"][ctx]) == 2
        for e in out["catalog"][ctx]:
            uuid[os.path.basename(e["name"])] = e["uuid"]
            ctx_of[e["uuid"]] = (ctx, os.path.basename(e["name"]))
    # the mirror: one engine holding the prompts under the catalog's uuids, context "a" as scope 0, "b" as 1
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
            rows, fc, ff = lv.window(p, [0, 1], K, frames)
            for c in range(2):
                ch = got["channels"][c]
                F = tfp_lib.frame_count(lv.samples(c))
                assert (ch["first_frame"], ch["frame_count"]) == (ff[c], fc[c]) == (max(0, F - frames), min(F, frames)), (at, ms, c)
                assert [(x["uuid"], x["match_count"]) for x in ch["rows"]] == \
                    [(x["audio_uuid"], x["match_count"]) for x in rows[c]], (at, ms, c)
                for x in ch["rows"]:  # the catalog's fields of the row's clip, in the channel's context
                    assert (x["context"], os.path.basename(x["name"])) == ctx_of[x["uuid"]] and x["context"] == "ab"[c]
                    assert x["frame_count"] == fc[c] and x["hash"]
                some_rows += len(ch["rows"])
        assert lv.samples(0) == 3200 and lv.samples(1) == 3000 and some_rows
        st = lv.window_stats()
        assert st["slid_calls"] == len(ASKS) and st["general_calls"] == 0
        lv.close()
    finally:
        engine.index_clear()
