"""Ranked search at the module's facade: fp_search_fingerprint_candidates of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_ranked_harness.c) and of the Python mirror
(tiresias_amd.fp_handler.FpHandler): the result query's first rows (fp_handler.c:367-374) as the
objects fp_search_fingerprint_info returns, in rank order, checked against a brute-force count."""
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


def _expected(oracle, pcm, uuids, query):
    rows = [oracle.fingerprint(p)[2] for p in pcm]
    micro = np.concatenate(rows)
    clip = np.repeat(np.arange(len(pcm)), len(rows[0]))
    _, qdb, _ = oracle.fingerprint(query)
    return R.brute_force(oracle, uuids, clip, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), 1, 0.45, -1, -1), len(qdb)


def test_shim_candidates(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_ranked")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_ranked_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    pcm = tfp_lib.synth_pcm(SEED, range(3), 8000 * 8)
    files = []
    for c in range(3):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    query = pcm[2, 256 * 40: 256 * 40 + 24000]
    q = str(tmp_path / "q.wav")
    write_wav_mono16(q, query)
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), "ctx", "2", "1", "0.45", q, *files],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    cand = out["candidates"]
    uuid_of = {c["name"]: c["uuid"] for c in cand}
    # the module generated the uuids: the expected order with the returned clips' uuids in place
    names = ["clip%d.wav" % c for c in range(3)]
    by_name, nf = _expected(oracle, pcm, names, query)
    counts = dict(by_name)
    assert 2 <= len(by_name), "the query should score at least two clips"
    assert len(cand) == 2 and out["info"] == cand[0]
    assert all(c["frame_count"] == nf and c["match_count"] == counts[c["name"]] for c in cand)
    # rank order: count descending, tied counts by uuid descending; nothing left out scores above the second row
    keys = [(c["match_count"], c["uuid"]) for c in cand]
    assert keys == sorted(keys, reverse=True)
    left = [n for n in names if n not in uuid_of]
    assert all(counts.get(n, 0) <= cand[1]["match_count"] for n in left)
    assert cand[0]["match_count"] == by_name[0][1] and cand[1]["match_count"] == by_name[1][1]


def test_fp_handler_candidates(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    fp = FpHandler(0)
    assert fp.fp_init()
    try:
        pcm = tfp_lib.synth_pcm(SEED, range(6), 8000 * 8)
        for i in range(6):
            f = str(tmp_path / f"clip{i}.wav")
            write_wav_mono16(f, pcm[i])
            assert fp.fp_craete_audio_list_info("ctx", f)
        query = pcm[2, 256 * 40: 256 * 40 + 24000]
        q = str(tmp_path / "q.wav")
        write_wav_mono16(q, query)
        uu = {r["name"]: r["uuid"] for r in fp.fp_get_audio_lists_all()}
        uuids = [uu["clip%d.wav" % i] for i in range(6)]
        exp, nf = _expected(oracle, pcm, uuids, query)
        assert len(exp) >= 2
        for k in (1, 2, 32):
            got = fp.fp_search_fingerprint_candidates("ctx", q, 1, 0.45, -1, -1, k)
            assert [(g["uuid"], g["match_count"]) for g in got] == exp[:k]
            assert all(g["frame_count"] == nf and g["context"] == "ctx" and g["name"].startswith("clip") for g in got)
        assert got[0] == fp.fp_search_fingerprint_info("ctx", q, 1, 0.45, -1, -1)
        assert fp.fp_search_fingerprint_candidates("ctx", q, 3, 0.45, -1, -1, 2) == []
        assert fp.fp_search_fingerprint_candidates("ctx", str(tmp_path / "missing.wav"), 1, 0.45, -1, -1, 2) == []
        assert fp.fp_search_fingerprint_candidates(None, q, 1, 0.45, -1, -1, 2) == []
    finally:
        assert fp.fp_term()
