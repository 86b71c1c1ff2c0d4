"""The compiled shim's index rate (fp_set_index_rate in shim/fp_handler_tfp.c, driven from C by
tests/native/shim_index_rate_harness.c, run as a child process): with the rate set to 8000 the shim enrols a
directory of six files of different rates, channel counts and kinds plus one at 8000 through its mixed bucket, and
the backup it writes loads into the mirror with the rows of the mirror's own mixed enrolment; a 16 kHz mono
rendering of the prompt enrolled from a 44.1 kHz stereo master finds that prompt; a file at an unsupported ratio is
refused and leaves no catalog row; without the call the enrolment is today's, at native rates."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from resample_util import class_clip
from test_gpu_any_handler import _stereo, _ulaw_codes, _write_g711_wav, _write_wav

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]
NAMES = ["a_16k_mono16.wav", "b_44k_stereo16.wav", "c_48k_stereo24.wav", "d_44k_mono32.wav", "e_16k_ulaw.wav",
         "f_16k_stereo16.wav", "g_8k_mono16.wav"]


def _build(tmp_path, lib):
    exe = str(tmp_path / "shim_index_rate")
    stubs = str(tmp_path / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp_path / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_index_rate_harness.c"),
                    stubs, str(tmp_path / "fp_handler_tfp.c.o"), str(tmp_path / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    return exe


def _rows_by_name(h):
    return {r["name"]: h.engine.index_rows(r["uuid"]) for r in h.fp_get_audio_lists_all()}


def _mirror_rows(d, **kw):
    from tiresias_amd import FpHandler
    h = FpHandler(0, **kw)
    assert h.fp_init()
    try:
        assert h.fp_create_context_list_info("ctx", str(d), False) and h.create_new_audio_info("ctx")
        return _rows_by_name(h)
    finally:
        h.fp_term()


def _run(exe, tmp_path, tag, rate, query, bad, d):
    db = tmp_path / (tag + ".db")
    r = subprocess.run([exe, str(db), str(rate), "1", "0.45", str(query), str(bad), *[str(d / nm) for nm in NAMES]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.splitlines()[-1])
    from tiresias_amd import FpHandler
    h = FpHandler(0, backup_path=str(db))  # the backup the shim wrote, loaded into the mirror
    assert h.fp_init()
    try:
        return out, _rows_by_name(h)
    finally:
        h.backup_path = None  # (leave the shim's file as it is)
        h.fp_term()


def test_shim_index_rate(tmp_path, tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    exe = _build(tmp_path, os.path.dirname(tfp_lib.LIB_PATH))
    d = tmp_path / "prompts"
    d.mkdir()
    # the three clips the reference's search tells apart (resample_util.class_clip): b, the 44.1 kHz stereo master, is
    # the only file of its class
    src = [class_clip(2, 16000), class_clip(0, 16000), class_clip(1, 16000)] + [class_clip(k, 16000)[::-1].copy() for k in (1, 2, 1, 2)]
    up = lambda x, r: tfp_lib.resample_pcm(x, 8000, r)  # noqa: E731
    _write_wav(d / NAMES[0], up(src[0], 16000), 16000)
    _write_wav(d / NAMES[1], _stereo(up(src[1], 44100), 1), 44100)
    _write_wav(d / NAMES[2], _stereo(up(src[2], 48000), 2), 48000, width=3)
    _write_wav(d / NAMES[3], up(src[3], 44100), 44100, width=4)
    _write_g711_wav(d / NAMES[4], _ulaw_codes(tfp_lib, up(src[4], 16000)), 16000, 7)
    _write_wav(d / NAMES[5], _stereo(up(src[5], 16000), 3), 16000)
    _write_wav(d / NAMES[6], src[6], 8000)
    query = tmp_path / "heard_16k.wav"
    _write_wav(query, up(src[1][256 * 3:256 * 3 + 9000], 16000), 16000)  # the master's prompt, heard as 16 kHz mono
    bad = tmp_path / "z_44101.wav"
    _write_wav(bad, up(src[0], 16000), 44101)  # 44101 -> 8000: a table past the builder's limit
    with pytest.raises(tfp_lib.TfpError, match="unsupported rate ratio"):
        tfp_lib.resample_taps(44101, 8000)

    out, rows = _run(exe, tmp_path, "rate8000", 8000, query, bad, d)
    assert out["enrolled"] == 7 and out["ok"] == [1] * 7
    assert out["bad_scan"] == 0 and out["bad_single"] == 0 and sorted(rows) == sorted(NAMES)  # refused, no catalog row
    want = _mirror_rows(d, index_rate=8000, mix_channels=True, wide_samples=True, mixed_batch=True)
    assert sorted(want) == sorted(NAMES)
    for nm in NAMES:
        assert len(rows[nm][0]) == 63, nm  # 2 s at the index rate, whatever the file's own rate
        assert np.array_equal(rows[nm][0], want[nm][0]) and np.array_equal(rows[nm][1], want[nm][1]), nm
    assert out["query"] is not None and out["query"]["name"] == NAMES[1] and out["query"]["match_count"] > 0, out["query"]
    assert out["query"]["frame_count"] == tfp_lib.frame_count(9000)

    # without the call: the native-rate rows, as before the setting existed
    out0, rows0 = _run(exe, tmp_path, "rate0", 0, query, bad, d)
    assert out0["enrolled"] == 7 and out0["ok"] == [1] * 7
    native = _mirror_rows(d)
    for nm in NAMES:
        assert np.array_equal(rows0[nm][0], native[nm][0]) and np.array_equal(rows0[nm][1], native[nm][1]), nm
    assert len(rows0[NAMES[1]][0]) == tfp_lib.frame_count(len(up(src[1], 44100)))  # at 44.1 kHz: not the 8 kHz rows
