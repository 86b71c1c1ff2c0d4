"""The match census at the module's facade: fp_search_fingerprint_census of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_census_harness.c) against the Python mirror
(FpHandler.fp_search_fingerprint_census) and a brute-force count over each context's clips."""
import json
import os
import subprocess

import numpy as np
import pytest

import census_util as U
import ranked_util as R
from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1


def test_shim_census(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_census")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_census_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    pcm = tfp_lib.synth_pcm(SEED, range(6), 8000 * 8)
    files = []
    for c in range(6):
        files.append(str(tmp_path / ("clip%d.wav" % c)))
        write_wav_mono16(files[-1], pcm[c])
    query = pcm[2, 256 * 40: 256 * 40 + 24000]
    q = str(tmp_path / "q.wav")
    write_wav_mono16(q, query)
    # context a: clips 0-2; context b: clips 3-5 and clip 2 again (a second clip with its rows)
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), "1", "0.45", q, "3", *files[:3], *files[3:], files[2]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    # the counts, by the oracle's fingerprints and a brute-force count over each context's clips
    rows = [oracle.fingerprint(x)[2] for x in pcm]
    micro = np.concatenate(rows)
    clip = np.repeat(np.arange(6), len(rows[0]))
    _, qdb, _ = oracle.fingerprint(query)
    names = ["clip%d.wav" % c for c in range(6)]
    counts = dict(R.brute_force(oracle, names, clip, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), 1, 0.45,
                                -1, -1))
    F = len(qdb)
    for ctx, own in (("a", names[:3]), ("b", names[3:] + ["clip2.wav"])):
        got = out[ctx]
        mine = [counts.get(nm, 0) for nm in own]
        exp = U.dense(U.sparse([(None, n) for n in mine if n]), len(own), F + 1)
        assert got["histogram"] == [[c, int(exp[c])] for c in range(F, -1, -1) if exp[c]]
        assert got["frame_count"] == F and got["population"] == len(own) == sum(n for _, n in got["histogram"])
        top = max(mine)
        assert top > 0 and got["winner"] == got["first"] and got["winner"]["match_count"] == top
        assert got["winner"]["context"] == ctx and got["winner"]["name"] in own and got["winner"]["frame_count"] == F
        assert got["clips_tied"] == mine.count(top) == got["clips_at_or_above"]
    assert out["nowhere"] == {"winner": None, "first": None, "frame_count": F, "population": 0, "clips_at_or_above": 0,
                              "clips_tied": 0, "histogram": []}
    # the Python mirror gives the same fields
    fp = FpHandler(0, backup_path=str(tmp_path / "mirror.db"))
    assert fp.fp_init()
    for f in files[:3]:
        assert fp.fp_craete_audio_list_info("a", f)
    for f in files[3:] + [files[2]]:
        assert fp.fp_craete_audio_list_info("b", f)
    for ctx in ("a", "b", "nowhere"):
        m = fp.fp_search_fingerprint_census(ctx, q, 1, 0.45, -1, -1)
        for key in ("frame_count", "population", "clips_at_or_above", "clips_tied", "histogram"):
            assert m[key] == out[ctx][key], (ctx, key)
        if out[ctx]["winner"] is None:
            assert m["winner"] is None
        else:
            # (the two enrolments draw their own uuids, so among tied clips the winners' names may differ)
            assert (m["winner"]["context"], m["winner"]["match_count"], m["winner"]["frame_count"]) == \
                tuple(out[ctx]["winner"][k] for k in ("context", "match_count", "frame_count"))
            assert counts[m["winner"]["name"]] == counts[out[ctx]["winner"]["name"]] == m["winner"]["match_count"]
            first = fp.fp_search_fingerprint_in_context(ctx, q, 1, 0.45, -1, -1)
            assert m["winner"] == first[0]
    assert fp.fp_search_fingerprint_census("a", q, 3, 0.45, -1, -1) is None
    assert fp.fp_search_fingerprint_census("a", str(tmp_path / "missing.wav"), 1, 0.45, -1, -1) is None
    assert fp.fp_term()
