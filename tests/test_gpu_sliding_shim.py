"""Sliding search at the module's facade: fp_search_fingerprint_timeline of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_sliding_harness.c) and of the Python mirror
(tiresias_amd.fp_handler.FpHandler) agree with each other and with a brute-force count over the
oracle's fingerprints, window by window, on one recording: noise, an excerpt of an enrolled clip,
noise. With and without in_context."""
import json
import os
import subprocess

import numpy as np
import pytest

import ranked_util as R
from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1
WINDOW, HOP = 24, 6


def _key(rows):
    """Rows without their uuids (random per enrolment), in an order of their own."""
    return sorted((-r["match_count"], r["name"], r["context"], r["frame_count"]) for r in rows)


def test_shim_and_mirror_timeline(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_sliding")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_sliding_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    pcm = tfp_lib.synth_pcm(SEED, range(6), 8000 * 8)
    files = []
    for c in range(6):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    noise = tfp_lib.synth_pcm(0xBEEF, range(2), 256 * 60)
    # noise, 3 s of clip 2 from a frame boundary, noise: the excerpt's frames keep the clip's frame grid
    rec = np.concatenate([noise[0][:256 * 50], pcm[2, 256 * 40: 256 * 40 + 24000], noise[1][:256 * 45 + 100]])
    rw = str(tmp_path / "rec.wav")
    write_wav_mono16(rw, rec)
    # context a: clips 0-2 one by one; context b: clips 3-5 as a list
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), "1", "0.45", rw, str(WINDOW), str(HOP), "32", "3",
                        *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    shim = json.loads(r.stdout.splitlines()[-1])
    # the mirror, enrolled the same way
    fp = FpHandler(0)
    assert fp.fp_init()
    for c in range(6):
        assert fp.fp_craete_audio_list_info("a" if c < 3 else "b", files[c])
    mirror = {"all": fp.fp_search_fingerprint_timeline("a", rw, 1, 0.45, -1, -1, WINDOW, HOP, 32),
              "a": fp.fp_search_fingerprint_timeline("a", rw, 1, 0.45, -1, -1, WINDOW, HOP, 32, in_context=True),
              "b": fp.fp_search_fingerprint_timeline("b", rw, 1, 0.45, -1, -1, WINDOW, HOP, 32, in_context=True),
              "nowhere": fp.fp_search_fingerprint_timeline("nowhere", rw, 1, 0.45, -1, -1, WINDOW, HOP, 32, in_context=True)}
    assert fp.fp_search_fingerprint_timeline("a", rw, 1, 0.45, -1, -1, 100000, HOP, 32) == []
    assert fp.fp_search_fingerprint_timeline("a", rw, 1, 0.45, -1, -1, WINDOW, 0, 32) == []
    assert fp.fp_search_fingerprint_timeline("a", rw, 3, 0.45, -1, -1, WINDOW, HOP, 32) == []
    top1 = fp.fp_search_fingerprint_timeline("a", rw, 1, 0.45, -1, -1, WINDOW, HOP, 1)
    assert fp.fp_term()
    assert shim["long"] == [] and shim["bad"] is None
    # the oracle: the recording's own fingerprint, every window counted by brute force over the six clips
    rows = [oracle.fingerprint(p)[2] for p in pcm]
    micro = np.concatenate(rows)
    clip = np.repeat(np.arange(6), len(rows[0]))
    _, qdb, _ = oracle.fingerprint(rec)
    names = ["clip%d.wav" % c for c in range(6)]
    ctx_of = {n: ("a" if c < 3 else "b") for c, n in enumerate(names)}
    nw = (len(qdb) - WINDOW) // HOP + 1
    assert nw > 20
    best = []
    for key in ("all", "a", "b", "nowhere"):
        assert len(shim[key]) == len(mirror[key]) == nw, key
    for w in range(nw):
        a = w * HOP
        counts = R.brute_force(oracle, names, clip, micro[:, 0], micro[:, 1], list(qdb[a:a + WINDOW, 0]),
                               list(qdb[a:a + WINDOW, 1]), 1, 0.45, -1, -1)
        for key in ("all", "a", "b", "nowhere"):
            want = sorted((-n, u, ctx_of[u], WINDOW) for u, n in counts if key == "all" or ctx_of[u] == key)
            for side in (shim, mirror):
                assert side[key][w]["frame"] == a
                assert _key(side[key][w]["rows"]) == want, (key, w)
                cs = [(c["match_count"], c["uuid"]) for c in side[key][w]["rows"]]
                assert cs == sorted(cs, reverse=True)  # count descending, tied counts by uuid descending
        assert top1[w]["rows"] == mirror["all"][w]["rows"][:1]
        best.append(counts[0] if counts else None)
    assert sum(b is not None for b in best) > nw // 2  # the recording does find clips
