"""Occurrence search at the module's facade: fp_search_fingerprint_occurrences of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_occurrences_harness.c) and of the Python mirror
(tiresias_amd.fp_handler.FpHandler) agree with each other, every occurrence they report is the oracle's trace
of its diagonal, and the enrolled excerpt inside a longer recording comes out as one occurrence that names the
excerpt's place and reaches its ends."""
import json
import os
import subprocess

import numpy as np
import pytest

import align_util as A
import occurrence_util as O
from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1
# As test_gpu_sliding_aligned_shim.py: at tolerance 0.999 every frame hits its own stored row (fp_handler.c:290), and
# 48 frames of a clip whose level moves from hop to hop fit it in one place. max1 of 8 kHz audio spans about 1 dB,
# so a noise frame still hits about half of any clip's rows: with max_gap 0 the excerpt's diagonal is one unbroken
# segment over the excerpt and breaks up in the noise around it.
WINDOW, HOP, K, MAX_GAP, MIN_HITS = 48, 6, 32, 0, 20
COEFS, TOL = 1, 0.999
NOISE_FRAMES, CLIP_FRAME0, EXCERPT_FRAMES = 50, 40, 187
FIELDS = ("clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap", "windows")


def _key(rows):
    """Occurrences without their uuids (random per enrolment, and they order the ties), in an order of their own."""
    return sorted((r["name"], r["context"], r["frame_count"], r["match_count"]) + tuple(r[k] for k in FIELDS) for r in rows)


def test_shim_and_mirror_occurrences(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_occurrences")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", *INC,
                    os.path.join(NATIVE, "shim_occurrences_harness.c"), stubs, str(tmp_path / "fp_handler_tfp.c.o"),
                    str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib, "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS],
                   check=True)
    pcm = tfp_lib.synth_pcm(SEED, range(6), 8000 * 8)
    rng = np.random.default_rng(SEED)  # clip 2: noise of a level of its own in every hop
    hops = pcm.shape[1] // 256
    gain = np.repeat(10 ** rng.uniform(-2.7, 0, hops), 256)
    pcm[2, :hops * 256] = np.clip(rng.normal(size=hops * 256) * 7000 * gain, -32767, 32767).astype(np.int16)
    files = []
    for c in range(6):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    # faint noise, 6 s of clip 2 from a frame boundary, faint noise: the excerpt's frames keep the clip's frame grid
    noise = np.round(np.random.default_rng(0xBEEF).normal(size=256 * 110)).astype(np.int16)
    rec = np.concatenate([noise[:256 * NOISE_FRAMES], pcm[2, 256 * CLIP_FRAME0: 256 * (CLIP_FRAME0 + EXCERPT_FRAMES)],
                          noise[256 * NOISE_FRAMES:256 * 95 + 100]])
    rw = str(tmp_path / "rec.wav")
    write_wav_mono16(rw, rec)
    # context a: clips 0-2 one by one; context b: clips 3-5 as a list
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), str(COEFS), str(TOL), rw, str(WINDOW), str(HOP), str(K),
                        str(MAX_GAP), str(MIN_HITS), "3", *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    shim = json.loads(r.stdout.splitlines()[-1])
    fp = FpHandler(0)  # the mirror, enrolled the same way
    assert fp.fp_init()
    for c in range(6):
        assert fp.fp_craete_audio_list_info("a" if c < 3 else "b", files[c])
    args = (rw, COEFS, TOL, -1, -1, WINDOW, HOP, K, MAX_GAP)
    mirror = {key: fp.fp_search_fingerprint_occurrences(key, *args, MIN_HITS) for key in ("a", "b", "nowhere")}
    assert fp.fp_search_fingerprint_occurrences("a", rw, COEFS, TOL, -1, -1, 100000, HOP, K, MAX_GAP, MIN_HITS) == []
    assert fp.fp_search_fingerprint_occurrences("a", *args, 0) == []
    assert fp.fp_search_fingerprint_occurrences("a", *args, 100000) == []
    assert fp.fp_search_fingerprint_occurrences("a", rw, COEFS, TOL, -1, -1, WINDOW, HOP, K, -1, MIN_HITS) == []
    assert fp.fp_term()
    assert shim["long"] == [] and shim["bad"] is None and shim["strict"] == [] and shim["nowhere"] == mirror["nowhere"] == []
    qdb = oracle.fingerprint(rec)[1]
    nf = len(qdb)
    assert nf == tfp_lib.frame_count(len(rec))
    hits = {}
    for key, clips in (("a", range(3)), ("b", range(3, 6))):
        assert _key(shim[key]) == _key(mirror[key]) and len(mirror[key]) >= 1, key  # the JSON equals the mirror's list
        for side in (shim[key], mirror[key]):
            assert [o["first_frame"] for o in side] == sorted(o["first_frame"] for o in side)
            for o in side:  # every occurrence is the oracle's trace of its diagonal, and a clip of its context
                c = int(o["name"][4])
                assert c in clips and o["context"] == key and o["frame_count"] == nf and o["match_count"] == o["hits"] >= MIN_HITS
                if c not in hits:
                    micro = oracle.fingerprint(pcm[c])[2]
                    hits[c] = A.hit_matrix(oracle, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), COEFS, TOL, -1, -1)
                t = O.trace_of_hits(hits[c], o["clip_start_frame"], MAX_GAP)
                assert (o["overlap"], o["diagonal_hits"], o["hits"], o["first_frame"], o["last_frame"]) == \
                    (t[0], t[1], t[3], t[4], t[5]), o
                assert o["windows"] >= 1
    # the excerpt: recording frame 50 is clip frame 40, so clip frame 0 lies at recording frame 10; its segment runs
    # from the excerpt's first frame, or the next (the first one's analysis window still sees the noise), to its last
    # frame, or the next (whose analysis window still sees the excerpt)
    start, end = NOISE_FRAMES - CLIP_FRAME0, NOISE_FRAMES + EXCERPT_FRAMES - 1
    for side in (shim["a"], mirror["a"]):
        best = max((o for o in side if o["name"] == "clip2.wav"), key=lambda o: o["hits"])
        assert best["clip_start_frame"] == start and best["windows"] >= 20
        assert NOISE_FRAMES <= best["first_frame"] <= NOISE_FRAMES + 1 and end <= best["last_frame"] <= end + 1, best
        assert best["hits"] == best["last_frame"] - best["first_frame"] + 1  # unbroken
