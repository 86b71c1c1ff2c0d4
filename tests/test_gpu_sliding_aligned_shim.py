"""Sliding aligned search at the module's facade: fp_search_fingerprint_timeline_aligned of the compiled
shim (shim/fp_handler_tfp.c, driven from C by tests/native/shim_sliding_aligned_harness.c) and of the
Python mirror (tiresias_amd.fp_handler.FpHandler) agree with each other, with the timeline call's rows,
and with the excerpt's place: every window of an enrolled excerpt inside a longer synthetic recording
equals the oracle's brute-force alignment and reports one clip_start_frame. With and without in_context."""
import json
import os
import subprocess

import numpy as np
import pytest

import align_util as A
from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1
# A frame hits its own stored row when max1 lies within the tolerance of its truncated key (fp_handler.c:290): at
# 0.999 every frame does. 8 kHz audio gives max1 = 10 log10 |c0| a range of about 1 dB, so a short window fits its
# clip in several places; 48 frames of a clip whose level moves from hop to hop fit in one (asserted below on the
# oracle's own fingerprints, before anything is asked of the shim)
WINDOW, HOP = 48, 6
COEFS, TOL = 1, 0.999
NOISE_FRAMES, CLIP_FRAME0, EXCERPT_FRAMES = 50, 40, 187
EXTRA = ("aligned_count", "offset", "first_frame", "last_frame", "clip_start_frame")


def _key(rows):
    """Rows without their uuids (random per enrolment, and they order the tied counts), in an order of their own."""
    return sorted((-r["match_count"], r["name"], r["context"], r["frame_count"]) + tuple(r[k] for k in EXTRA) for r in rows)


def test_shim_and_mirror_timeline_aligned(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_sliding_aligned")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC,
                    os.path.join(NATIVE, "shim_sliding_aligned_harness.c"), stubs, str(tmp_path / "fp_handler_tfp.c.o"),
                    str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib, "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS],
                   check=True)
    pcm = tfp_lib.synth_pcm(SEED, range(6), 8000 * 8)
    # clip 2 is noise of a level of its own in every hop (over 54 dB), which moves max1's truncated key from frame to
    # frame as far as the log of a log lets it
    rng = np.random.default_rng(SEED)
    hops = pcm.shape[1] // 256
    gain = np.repeat(10 ** rng.uniform(-2.7, 0, hops), 256)
    pcm[2, :hops * 256] = np.clip(rng.normal(size=hops * 256) * 7000 * gain, -32767, 32767).astype(np.int16)
    files = []
    for c in range(6):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    noise = tfp_lib.synth_pcm(0xBEEF, range(2), 256 * 60)
    # noise, 6 s of clip 2 from a frame boundary, noise: the excerpt's frames keep the clip's frame grid
    rec = np.concatenate([noise[0][:256 * NOISE_FRAMES], pcm[2, 256 * CLIP_FRAME0: 256 * (CLIP_FRAME0 + EXCERPT_FRAMES)],
                          noise[1][:256 * 45 + 100]])
    rw = str(tmp_path / "rec.wav")
    write_wav_mono16(rw, rec)
    # context a: clips 0-2 one by one; context b: clips 3-5 as a list
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), str(COEFS), str(TOL), rw, str(WINDOW), str(HOP), "32", "3",
                        *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    shim = json.loads(r.stdout.splitlines()[-1])
    # the mirror, enrolled the same way
    fp = FpHandler(0)
    assert fp.fp_init()
    for c in range(6):
        assert fp.fp_craete_audio_list_info("a" if c < 3 else "b", files[c])
    args = (rw, COEFS, TOL, -1, -1, WINDOW, HOP, 32)
    mirror = {"all": fp.fp_search_fingerprint_timeline_aligned("a", *args),
              "a": fp.fp_search_fingerprint_timeline_aligned("a", *args, in_context=True),
              "b": fp.fp_search_fingerprint_timeline_aligned("b", *args, in_context=True),
              "nowhere": fp.fp_search_fingerprint_timeline_aligned("nowhere", *args, in_context=True)}
    plain = {"all": fp.fp_search_fingerprint_timeline("a", *args),
             "b": fp.fp_search_fingerprint_timeline("b", *args, in_context=True)}
    assert fp.fp_search_fingerprint_timeline_aligned("a", rw, COEFS, TOL, -1, -1, 100000, HOP, 32) == []
    assert fp.fp_search_fingerprint_timeline_aligned("a", rw, COEFS, TOL, -1, -1, WINDOW, 0, 32) == []
    assert fp.fp_search_fingerprint_timeline_aligned("a", rw, 3, TOL, -1, -1, WINDOW, HOP, 32) == []
    assert fp.fp_term()
    assert shim["long"] == [] and shim["bad"] is None
    nw = (len(rec) // 256 - WINDOW) // HOP + 1
    for key in ("all", "a", "b", "nowhere"):
        assert len(shim[key]) == len(mirror[key]) == nw > 20, key
        for w in range(nw):
            assert shim[key][w]["frame"] == mirror[key][w]["frame"] == w * HOP
            assert _key(shim[key][w]["rows"]) == _key(mirror[key][w]["rows"]), (key, w)  # the JSON equals the mirror's
            for row in mirror[key][w]["rows"]:
                assert 1 <= row["aligned_count"] <= row["match_count"] <= row["frame_count"] == WINDOW
                assert 0 <= row["first_frame"] <= row["last_frame"] < WINDOW
                assert row["clip_start_frame"] == w * HOP - row["offset"]
    assert all(not win["rows"] for win in mirror["nowhere"])
    # the timeline call's array, with five more integers per row
    for key in plain:
        assert [[{k: v for k, v in r.items() if k not in EXTRA} for r in win["rows"]] for win in mirror[key]] == \
            [win["rows"] for win in plain[key]]
    # the windows inside the excerpt, past its first frame (whose analysis window still sees the noise): their
    # frames are the clip's own, so clip 2 has every frame on the diagonal of the occurrence, recording frame 50 =
    # clip frame 40, clip_start_frame 10. The expected rows come from the oracle's fingerprints and the brute
    # force, which also says that no other diagonal of any of these windows reaches the count
    inside = [w for w in range(nw) if NOISE_FRAMES + 1 <= w * HOP and w * HOP + WINDOW <= NOISE_FRAMES + EXCERPT_FRAMES]
    assert len(inside) >= 20
    micro = oracle.fingerprint(pcm[2])[2]
    qdb = oracle.fingerprint(rec)[1]
    ref = [A.brute_force(oracle, micro[:, 0], micro[:, 1], list(qdb[w * HOP:w * HOP + WINDOW, 0]),
                         list(qdb[w * HOP:w * HOP + WINDOW, 1]), COEFS, TOL, more=True) for w in inside]
    want = [four for four, _, _ in ref]
    start = NOISE_FRAMES - CLIP_FRAME0
    assert not any(tie for _, _, tie in ref)
    assert all(f == (WINDOW, w * HOP - start, 0, WINDOW - 1) for w, f in zip(inside, want))
    for side in (shim, mirror):
        for key in ("all", "a"):
            rows = [next(r for r in side[key][w]["rows"] if r["name"] == "clip2.wav") for w in inside]
            assert [tuple(r[k] for k in EXTRA[:4]) for r in rows] == want, key
            assert all(r["match_count"] == WINDOW for r in rows)
            assert [r["clip_start_frame"] for r in rows] == [start] * len(inside), key  # one occurrence, one value
