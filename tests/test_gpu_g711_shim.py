"""G.711 at the module's facade: the compiled shim (shim/fp_handler_tfp.c, driven from C by
tests/native/shim_g711_harness.c) enrols a directory holding an int16 WAV, a mu-law WAV, headerless
.ulaw and .alaw files and a stereo PCM WAV in one fp_create_audio_list_infos scan, finds each file by
a search of itself, and fp_channel_push_g711 + fp_channel_search equals the search of the expanded
recording."""
import json
import os
import subprocess
import wave

import numpy as np
import pytest

import ranked_util as R
from conftest import REPO
from g711_util import ALAW, ULAW, encode, expand, g711_wav

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
SEED = 0x7153A1


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_g711")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_g711_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    return exe


def test_shim_g711(tmp_path, tfp_lib, oracle):
    from tiresias_amd.fp_handler import write_wav_mono16
    exe = _build(tmp_path, os.path.dirname(tfp_lib.LIB_PATH))
    d = tmp_path / "prompts"
    d.mkdir()
    n = 8000 * 4
    pcm = tfp_lib.synth_pcm(SEED, range(5), n)
    names = ["a_int16.wav", "b_tag7.wav", "c_raw.ulaw", "d_raw.alaw", "e_stereo.wav"]
    write_wav_mono16(str(d / names[0]), pcm[0])
    (d / names[1]).write_bytes(g711_wav(encode(pcm[1], ULAW), ULAW))
    (d / names[2]).write_bytes(encode(pcm[2], ULAW).tobytes())
    (d / names[3]).write_bytes(encode(pcm[3], ALAW).tobytes())
    stereo = np.stack([pcm[4], pcm[4] // 3], 1).astype("<i2")
    with wave.open(str(d / names[4]), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(stereo.tobytes())
    # what aubio_source hands out for each file, and its oracle rows
    heard = [pcm[0], expand(encode(pcm[1], ULAW), ULAW), expand(encode(pcm[2], ULAW), ULAW),
             expand(encode(pcm[3], ALAW), ALAW)]
    fps = [oracle.fingerprint(x) for x in heard] + [oracle.fingerprint_f32(oracle.wav_mono_f32(stereo, 16))]
    micro = np.concatenate([f[2] for f in fps])
    nf = len(fps[0][2])
    clip = np.repeat(np.arange(5), nf)
    # a channel plays 3 s of the mu-law WAV's clip from a hop boundary, as mu-law payload
    rec_codes = encode(pcm[1], ULAW)[256 * 9:256 * 9 + 24000]
    (tmp_path / "payload.bin").write_bytes(rec_codes.tobytes())
    write_wav_mono16(str(tmp_path / "recording.wav"), expand(rec_codes, ULAW))
    coefs, tol = 1, 1.0
    r = subprocess.run([exe, str(tmp_path / "audio_recongition.db"), str(coefs), str(tol), str(ULAW),
                        str(tmp_path / "payload.bin"), str(tmp_path / "recording.wav"), *[str(d / nm) for nm in names]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.splitlines()[-1])

    def expected(qdb):
        """(match_count of the winner, its name if no other clip ties with it) by a brute-force count."""
        rows = R.brute_force(oracle, names, clip, micro[:, 0], micro[:, 1], list(qdb[:, 0]), list(qdb[:, 1]), coefs, tol, -1, -1)
        counts = dict(rows)
        top = max(counts.values())
        winners = [nm for nm, c in counts.items() if c == top]
        return counts, top, winners

    # Each file is found by a search of itself: at tolerance 1 every frame with a max1 has its own row
    # in its box ([k - 1, k + 1] around k = (int)max1, fp_handler.c:287-351), so no clip beats the file.
    for i, nm in enumerate(names):
        counts, top, winners = expected(fps[i][1])
        got = out["files"][i]
        assert got is not None and got["context"] == "ctx" and got["frame_count"] == nf, (nm, got)
        assert counts[nm] == top == got["match_count"] and got["name"] in winners, (nm, got, counts)
        if len(winners) == 1:
            assert got["name"] == nm
    # the channel fed G.711 payload equals the search of the expanded recording, and the oracle
    _, qdb, _ = oracle.fingerprint(expand(rec_codes, ULAW))
    counts, top, winners = expected(qdb)
    assert out["channel"] is not None and out["channel"] == out["recording"]
    assert out["channel"]["match_count"] == top and out["channel"]["name"] in winners
    assert out["channel"]["frame_count"] == len(qdb) == 94
