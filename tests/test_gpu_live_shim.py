"""Live calls at the module's facade: fp_live_open / fp_live_push_g711 / fp_live_verdict of the compiled
shim (shim/fp_handler_tfp.c, driven from C by tests/native/shim_live_harness.c). 4 prompts in two
contexts, two channels pushed as mu-law payload: the verdict's JSON at mid-call and at the end equals
the rule of tiresias_fp.h over the CPU oracle's counts (verdict_util), and the end's fields equal
fp_search_fingerprint_in_context on a WAV of the same samples (application_handler.c:152-185, :163)."""
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
PROMPTS = {"a": (V.ZLEAD, V.ZRIVAL), "b": (V.LONE, 5)}  # per context: the clip its call plays, and one of another kind
DURATION_MS, MID_TICK = 500, 16
FIELDS = ("uuid", "name", "context", "hash", "match_count", "frame_count")


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_live")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_live_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    return exe


def test_shim_live_verdict(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import write_wav_mono16
    exe = _build(tmp_path, os.path.dirname(tfp_lib.LIB_PATH))
    total = 8 * DURATION_MS
    files, clips = [], []
    for ctx in ("a", "b"):
        for c in PROMPTS[ctx]:
            files.append(str(tmp_path / ("%s_clip%d.wav" % (ctx, c))))
            write_wav_mono16(files[-1], V.clip_pcm(c))
            clips.append((ctx, c))
    heard, args = [], []
    for ch, ctx in enumerate(("a", "b")):
        codes = encode(V.clip_pcm(PROMPTS[ctx][0])[256:256 + total], ULAW)
        heard.append(expand(codes, ULAW).astype(np.int16))
        (tmp_path / ("ch%d.ulaw" % ch)).write_bytes(codes.tobytes())
        write_wav_mono16(str(tmp_path / ("ch%d.wav" % ch)), heard[-1])
    args = [str(tmp_path / n) for n in ("ch0.ulaw", "ch1.ulaw", "ch0.wav", "ch1.wav")]
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), str(V.TOL), str(DURATION_MS), str(MID_TICK), *args, *files],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout.splitlines()[-1])
    # the oracle's DB: the prompts' fingerprints under the uuids the catalog gave them
    uuid = {}
    for ctx in ("a", "b"):
        assert len(out["catalog"][ctx]) == 2
        for e in out["catalog"][ctx]:
            uuid[os.path.basename(e["name"])] = e["uuid"]
    rows = [oracle.fingerprint(V.clip_pcm(c))[2] for _, c in clips]
    d = {"uuids": [uuid[os.path.basename(f)] for f in files], "clip": np.repeat(np.arange(4), [len(x) for x in rows]),
         "m1": np.concatenate(rows)[:, 0].astype(np.int64), "m2": np.concatenate(rows)[:, 1].astype(np.int64),
         "scope": [0, 0, 1, 1]}
    early = 0
    for when, S in (("mid", MID_TICK * 160), ("end", total)):
        for ch in range(2):
            exp = V.verdict(oracle, d, heard[ch][:S], total, V.TOL, ch, [0, 1, 2, 3])
            got = out[when][ch]
            assert (got["decided"], got["complete"], got["remaining"]) == (int(exp["decided"]), int(exp["complete"]), exp["remaining"])
            assert got["rival_match_count"] == (exp["rival"][1] if exp["rival"] else -1), (when, ch)
            assert exp["leader"] is not None and (got["uuid"], got["match_count"]) == exp["leader"], (when, ch)
            assert got["frame_count"] == oracle.frame_count(S) and got["context"] == "ab"[ch]
            assert os.path.basename(got["name"]) == os.path.basename(files[2 * ch])  # the prompt the call plays
            early += when == "mid" and got["decided"] and not got["complete"]
    assert early  # a verdict before the recording is complete
    for ch in range(2):  # the end: what the application's search of the recording returns
        assert out["search"][ch] is not None
        assert {k: out["end"][ch][k] for k in FIELDS} == {k: out["search"][ch][k] for k in FIELDS}, ch
        assert out["end"][ch]["decided"] == 1 and out["end"][ch]["complete"] == 1 and out["end"][ch]["remaining"] == 0
