"""Aligned search at the module's facade: fp_search_fingerprint_aligned of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_aligned_harness.c) and of the Python mirror
(tiresias_amd.fp_handler.FpHandler): fp_search_fingerprint_candidates' rows in rank order, each with
aligned_count, offset, first_frame and last_frame, checked against the brute force over the CPU
oracle's fingerprints."""
import json
import os
import subprocess

import pytest

import align_util as A
from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1
D0, NFQ = 40, 90  # the query: frames 40..129 of clip 2 (whole hops; only its first frame lacks its window history)
TOL = 1.0  # (a stored value always lies within 1 dB of its own truncation: the true diagonal is full)


def _audio(tfp_lib, n):
    pcm = tfp_lib.synth_pcm(SEED, range(n), 8000 * 8)
    return pcm, pcm[2, 256 * D0: 256 * (D0 + NFQ)]


def _expected(oracle, clip_pcm, query):
    """The alignment of the query with one clip, from the CPU oracle's fingerprints."""
    micro = oracle.fingerprint(clip_pcm)[2]
    _, qdb, _ = oracle.fingerprint(query)
    return A.brute_force(oracle, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), 1, TOL)


def test_shim_aligned(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_aligned")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_aligned_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    pcm, query = _audio(tfp_lib, 3)
    files = []
    for c in range(3):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    q = str(tmp_path / "q.wav")
    write_wav_mono16(q, query)
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), "ctx", "3", "1", repr(TOL), q, *files],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    cand, al = out["candidates"], out["aligned"]
    assert len(al) == len(cand) >= 2
    keys = ("uuid", "name", "frame_count", "match_count")
    assert [{k: a[k] for k in keys} for a in al] == cand  # the candidates' rows, in rank order
    for a in al:
        c = int(a["name"][4])
        assert A.four(a) == _expected(oracle, pcm[c], query), a["name"]
        assert 1 <= a["aligned_count"] <= a["match_count"] <= a["frame_count"] == NFQ
    mine = next(a for a in al if a["name"] == "clip2.wav")
    assert mine["offset"] == D0 and mine["aligned_count"] >= NFQ - 1


def test_fp_handler_aligned(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    fp = FpHandler(0)
    assert fp.fp_init()
    try:
        pcm, query = _audio(tfp_lib, 4)
        for i in range(4):
            f = str(tmp_path / f"clip{i}.wav")
            write_wav_mono16(f, pcm[i])
            assert fp.fp_craete_audio_list_info("ctx", f)
        q = str(tmp_path / "q.wav")
        write_wav_mono16(q, query)
        for k in (1, 2, 32):
            got = fp.fp_search_fingerprint_aligned("ctx", q, 1, TOL, -1, -1, k)
            cand = fp.fp_search_fingerprint_candidates("ctx", q, 1, TOL, -1, -1, k)
            assert [{f: g[f] for f in c} for g, c in zip(got, cand)] == cand and len(got) == len(cand) == min(k, 4)
            for g in got:
                assert A.four(g) == _expected(oracle, pcm[int(g["name"][4])], query), g["name"]
        mine = next(g for g in got if g["name"] == "clip2.wav")
        assert mine["offset"] == D0 and mine["aligned_count"] >= NFQ - 1
        assert fp.fp_search_fingerprint_aligned("ctx", q, 3, TOL, -1, -1, 2) == []
        assert fp.fp_search_fingerprint_aligned("ctx", str(tmp_path / "missing.wav"), 1, TOL, -1, -1, 2) == []
        assert fp.fp_search_fingerprint_aligned(None, q, 1, TOL, -1, -1, 2) == []
    finally:
        assert fp.fp_term()
