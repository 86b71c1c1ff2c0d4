"""Context-scoped search at the module's facade: fp_search_fingerprint_in_context of the compiled shim
(shim/fp_handler_tfp.c, driven from C by tests/native/shim_scoped_harness.c): the result query's first
rows (fp_handler.c:367-374) over one context's clips, against fp_search_fingerprint_candidates' rows
and a brute-force count, before and after an fp_term / fp_init restart."""
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


def test_shim_in_context(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import write_wav_mono16
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp_path / "shim_scoped")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_scoped_harness.c"),
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
    # context a: clips 0-2 one by one; context b: clips 3-5 and clip 2 again (a second clip with its rows), as a list
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), "1", "0.45", q, "3", *files[:3], *files[3:], files[2]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    before = out["before"]
    every = before["all"]
    assert len(every) >= 3 and {c["context"] for c in every} == {"a", "b"}
    # the counts, by the oracle's fingerprints and a brute-force count over the seven enrolled clips
    rows = [oracle.fingerprint(p)[2] for p in pcm]
    micro = np.concatenate(rows)
    clip = np.repeat(np.arange(6), len(rows[0]))
    _, qdb, _ = oracle.fingerprint(query)
    names = ["clip%d.wav" % c for c in range(6)]
    counts = dict(R.brute_force(oracle, names, clip, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), 1, 0.45,
                                -1, -1))
    assert all(c["frame_count"] == len(qdb) and c["match_count"] == counts[c["name"]] for c in every)
    assert sorted(c["name"] for c in every) == sorted([n for n in names if n in counts] + ["clip2.wav"] * ("clip2.wav" in counts))
    keys = [(c["match_count"], c["uuid"]) for c in every]
    assert keys == sorted(keys, reverse=True)  # count descending, tied counts by uuid descending
    two = [c for c in every if c["name"] == "clip2.wav"]
    assert sorted(c["context"] for c in two) == ["a", "b"]
    # each context's rows are the unscoped rows of that context, in their order
    for ctx, own in (("a", names[:3]), ("b", names[3:] + ["clip2.wav"])):
        assert before[ctx] == [c for c in every if c["context"] == ctx]
        assert before[ctx] and all(c["name"] in own for c in before[ctx])
    assert before["nowhere"] == []
    assert out["after"] == before  # the scopes come back from audio_list's contexts at fp_init
