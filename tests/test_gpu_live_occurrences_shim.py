"""The calls' logs at the module's facade: fp_live_occurrences of the compiled shim (shim/fp_handler_tfp.c,
driven from C by tests/native/shim_live_occurrences_harness.c) over a group of three engines on device 0
("0,0,0"). Asked after every second tick, each channel's JSON array equals the entries of Live.occurrences of
the ctypes mirror, on an engine that holds the same prompts and took the same samples, joined with the
catalog; window_ms and max_gap_ms convert to frames as tfp_live_window_frames does (225 ms: 8 frames, 33 ms:
2 frames). NULL for window_ms <= 0, max_gap_ms < 0, min_hits < 1 and k < 1 (checked by the harness)."""
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
WINDOW_MS, GAP_MS, MIN_HITS, EVERY = 225, 33, 2, 2
WINDOW, GAP = 8, 2  # ceil(ms * 8 / 256)
SEVEN = ("clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap", "windows")


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_live_occurrences")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC,
                    os.path.join(NATIVE, "shim_live_occurrences_harness.c"), stubs, str(tmp_path / "fp_handler_tfp.c.o"),
                    str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib, "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS],
                   check=True)
    return exe


def test_shim_live_occurrences(tmp_path, tfp_lib, engine):
    from tiresias_amd.fp_handler import write_wav_mono16
    assert tfp_lib.lib().tfp_live_window_frames(WINDOW_MS, 8000) == WINDOW and tfp_lib.lib().tfp_live_window_frames(GAP_MS, 8000) == GAP
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
                        str(tmp_path / "ch1.ulaw"), *files, str(WINDOW_MS), str(GAP_MS), str(MIN_HITS), str(EVERY)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout.splitlines()[-1])
    cat = {e["uuid"]: (os.path.basename(e["name"]), ctx) for ctx in ("a", "b") for e in out["catalog"][ctx]}
    uuid = {name: u for u, (name, _) in cat.items()}
    engine.index_clear()
    try:
        for f, (ctx, c) in zip(files, clips):
            fr = engine.fingerprint(V.clip_pcm(c))
            engine.index_add(uuid[os.path.basename(f)], fr["m1"], fr["m2"])
        engine.index_set_scope([uuid[os.path.basename(f)] for f in files], [0, 0, 1, 1])
        lv = tfp_lib.Live(engine, 2, 16000)
        p = tfp_lib.params(1, V.TOL)
        nticks = max(-(-len(h) // 160) for h in heard)
        assert [a["tick"] for a in out["asks"]] == list(range(EVERY, nticks + 1, EVERY))
        entries = 0
        asks = iter(out["asks"])
        for tick in range(nticks):
            n = [max(0, min(160, len(h) - tick * 160)) for h in heard]
            blk = np.zeros((2, 160), np.int16)
            for c in range(2):
                blk[c, :n[c]] = heard[c][tick * 160:tick * 160 + n[c]]
            lv.push(blk, None, nsamples=n)
            if (tick + 1) % EVERY:
                continue
            got = next(asks)
            occ, _ = lv.occurrences(p, [0, 1], K, WINDOW, GAP, MIN_HITS, 64)
            for c in range(2):
                assert [x["uuid"] for x in got["log"][c]] == [o["audio_uuid"] for o in occ[c]], (tick, c)
                for x, o in zip(got["log"][c], occ[c]):
                    assert {f: x[f] for f in SEVEN} == {f: o[f] for f in SEVEN}, (tick, c)
                    assert (os.path.basename(x["name"]), x["context"]) == cat[x["uuid"]] and x["hash"]
                    assert x["context"] == "ab"[c]  # a channel's log holds its context's clips only
                entries += len(got["log"][c])
        assert entries
        lv.close()
    finally:
        engine.index_clear()
