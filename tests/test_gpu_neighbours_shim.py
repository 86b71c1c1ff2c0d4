"""Catalog neighbours at the module's facade: fp_get_audio_list_neighbours and fp_get_audio_neighbours of
the compiled shim (shim/fp_handler_tfp.c, driven from C by tests/native/shim_neighbours_harness.c) against
the Python mirror (tiresias_amd.fp_handler.FpHandler) loaded from the backup the shim wrote, so both hold
the same uuids: the JSON of a two-context catalog is equal, and a flush covers 512 audios (2 audios: one
tfp_group_index_neighbours call, 513: two, counted by tfp_neighbour_stats through fp_get_neighbour_stats).
The mirror itself is checked against the engine's rows joined with the catalog by hand."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(REPO, "tests", "native")
INC = ["-I" + os.path.join(REPO, d) for d in ("shim", "include", "tests/native/asterisk_stub")] + \
    ["-idirafter", "/opt/conda/include"]  # sqlite3.h (the image has libsqlite3.so.0 but no dev package)
LIBS = ["-l:libsqlite3.so.0", "-lcrypto", "-lm", "-lpthread"]


@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory, tfp_lib):
    tmp = tmp_path_factory.mktemp("shim_neighbours")
    lib = os.path.dirname(tfp_lib.LIB_PATH)
    exe = str(tmp / "shim_neighbours")
    stubs = str(tmp / "shim_harness.o")  # the Asterisk stubs of shim_harness.c, its driver's main renamed
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, "-Dmain=shim_driver_main", "-c",
                    os.path.join(NATIVE, "shim_harness.c"), "-o", stubs], check=True)
    for src in ("fp_handler_tfp.c", "fp_catalog.c"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", *INC, "-c",
                        os.path.join(REPO, "shim", src), "-o", str(tmp / (src + ".o"))], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", *INC, os.path.join(NATIVE, "shim_neighbours_harness.c"),
                    stubs, str(tmp / "fp_handler_tfp.c.o"), str(tmp / "fp_catalog.c.o"), "-o", exe, "-L" + lib,
                    "-ltiresias_fp", "-Wl,-rpath," + lib, *LIBS], check=True)
    return exe


def _shim_and_mirror(tmp_path, shim_exe, clips, na, coefs, tol, k):
    """The harness's JSON for the clips (the first na in context a, the rest in b), and the mirror's for the
    same catalog, loaded from the backup the shim wrote."""
    from tiresias_amd.fp_handler import FpHandler, write_wav_mono16
    files = []
    for i, x in enumerate(clips):
        files.append(str(tmp_path / ("clip%04d.wav" % i)))
        write_wav_mono16(files[-1], x)
    db = str(tmp_path / "audio_recongition.db")
    r = subprocess.run([shim_exe, db, str(coefs), repr(tol), str(k), str(na), *files], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.splitlines()[-1])
    fp = FpHandler(0, backup_path=db)
    assert fp.fp_init()
    try:
        first_b = fp.fp_get_audio_lists_by_contextname("b")[0]["uuid"]
        mirror = {c: fp.fp_get_audio_list_neighbours(c, coefs, tol, -1, -1, k) for c in ("a", "b", "nowhere")}
        mirror["one"] = fp.fp_get_audio_neighbours(first_b, coefs, tol, -1, -1, k)
    finally:
        fp.engine.close()  # (not fp_term: the backup stays as the shim wrote it)
        fp.engine = None
    return out, mirror


def test_shim_json_equals_the_mirrors_two_contexts(tmp_path, tfp_lib, shim_exe):
    pcm = tfp_lib.synth_pcm(SEED, range(3), 8000 * 4)
    clips = [pcm[0], pcm[1], pcm[0][256 * 10:], pcm[2], pcm[1][256 * 5:]]  # a: 0, 1, 0 trimmed; b: 2, 1 trimmed
    for coefs, tol, k in ((1, 1.0, 4), (2, 1.0, 32)):
        sub = tmp_path / ("c%d" % coefs)
        sub.mkdir()
        out, mirror = _shim_and_mirror(sub, shim_exe, clips, 3, coefs, tol, k)
        for key in ("a", "b", "nowhere", "one"):
            assert out[key] == mirror[key], key
        assert [len(out[c]) for c in ("a", "b", "nowhere")] == [3, 2, 0] and out["bad"] == 0
        assert out["calls"] == [1, 2, 3]  # one group call per context's flush, one for the single audio
        if coefs == 1:
            a = {g["name"]: g for g in out["a"]}
            orig = next(n for n in a["clip0002.wav"]["neighbours"] if n["name"] == "clip0000.wav")
            assert orig["offset"] == 10 and orig["aligned_count"] >= a["clip0002.wav"]["frame_count"] - 1
            assert all(n["context"] == "a" for g in out["a"] for n in g["neighbours"])
            assert out["one"]["name"] == "clip0003.wav" and out["one"]["context"] == "b"


def test_shim_flush_of_513_audios_is_two_group_calls(tmp_path, tfp_lib, shim_exe):
    pcm = np.random.default_rng(SEED + 1).integers(-3000, 3000, (515, 256 * 6)).astype(np.int16)  # (distinct files: MD5 dedup)
    out, mirror = _shim_and_mirror(tmp_path, shim_exe, list(pcm), 513, 1, 0.45, 2)
    assert len(out["a"]) == 513 and len(out["b"]) == 2
    assert out["calls"] == [2, 3, 4]  # 513 audios: two flushes; 2 audios: one; the single audio: one
    for key in ("a", "b", "one"):
        assert out[key] == mirror[key], key

SEED = 0x4E1B
FIELDS = ("match_count", "aligned_count", "offset", "first_frame", "last_frame")


# ---- the mirror against the engine


def _handler(tfp_lib):
    from tiresias_amd.fp_handler import FpHandler
    fp = FpHandler(0)
    assert fp.fp_init()
    return fp


def _enrol_rows(fp, context, name, m1, m2):
    """A catalog row and its fingerprint rows, as fp_craete_audio_list_info leaves them."""
    uuid = fp.fp_generate_uuid()
    fp.db.execute("insert into audio_list(uuid, name, context, hash) values (?, ?, ?, ?);", (uuid, name, context, "h" + name))
    fp.engine.index_add(uuid, np.asarray(m1, np.int32), np.asarray(m2, np.int32))
    fp.engine.index_set_scope([uuid], [fp._scope_of(context, True)])
    return uuid


def test_two_contexts_from_audio_files(tmp_path, tfp_lib):
    from tiresias_amd.fp_handler import write_wav_mono16
    fp = _handler(tfp_lib)
    try:
        pcm = tfp_lib.synth_pcm(SEED, range(3), 8000 * 4)
        clips = [pcm[0], pcm[1], pcm[2], pcm[0][256 * 10:], pcm[1][256 * 5:]]  # two trimmed lead-ins
        ctx = ["a", "a", "b", "a", "b"]
        for i, (x, c) in enumerate(zip(clips, ctx)):
            f = str(tmp_path / ("clip%d.wav" % i))
            write_wav_mono16(f, x)
            assert fp.fp_craete_audio_list_info(c, f)
        p = tfp_lib.params(1, 1.0)
        for context in ("a", "b"):
            got = fp.fp_get_audio_list_neighbours(context, 1, 1.0, -1, -1, 4)
            infos = fp.fp_get_audio_lists_by_contextname(context)
            assert [{k: g[k] for k in ("uuid", "name", "context", "hash")} for g in got] == infos
            res = fp.engine.index_neighbours([i["uuid"] for i in infos], p, 4, [fp._scope_of(context, False)] * len(infos))
            for g, r in zip(got, res):
                assert g["frame_count"] == r["frame_count"] > 0
                assert [(n["uuid"], *(n[f] for f in FIELDS)) for n in g["neighbours"]] == \
                    [(n["audio_uuid"], *(n[f] for f in FIELDS)) for n in r["neighbours"]]
                assert all(n["context"] == context and n["uuid"] != g["uuid"] for n in g["neighbours"])
        a = {g["name"]: g for g in fp.fp_get_audio_list_neighbours("a", 1, 1.0, -1, -1, 4)}
        orig = next(n for n in a["clip3.wav"]["neighbours"] if n["name"] == "clip0.wav")  # the trimmed copy's original
        assert orig["offset"] == 10 and orig["first_frame"] <= 1 and orig["aligned_count"] >= a["clip3.wav"]["frame_count"] - 1
        # one uuid across all contexts: clip 4 (context b) is clip 1 (context a) trimmed
        one = fp.fp_get_audio_neighbours(next(g["uuid"] for g in fp.fp_get_audio_lists_all() if g["name"] == "clip4.wav"),
                                         1, 1.0, -1, -1, 4)
        orig = next(n for n in one["neighbours"] if n["name"] == "clip1.wav")
        assert one["name"] == "clip4.wav" and orig["context"] == "a" and orig["offset"] == 5
        assert fp.fp_get_audio_neighbours("no-such-uuid", 1, 1.0, -1, -1, 4) is None
        assert fp.fp_get_audio_list_neighbours(None, 1, 1.0, -1, -1, 4) is None
        assert fp.fp_get_audio_list_neighbours("a", 3, 1.0, -1, -1, 4) is None
        assert fp.fp_get_audio_list_neighbours("nobody", 1, 1.0, -1, -1, 4) == []
    finally:
        fp.fp_term()


@pytest.mark.parametrize("n,calls", [(2, 1), (513, 2)])
def test_one_engine_call_per_512_audios(tfp_lib, n, calls):
    fp = _handler(tfp_lib)
    try:
        M = 10**6
        uu = [_enrol_rows(fp, "big", "a%04d" % i, [(i % 7) * M, (i % 5) * M, 9 * M], [0, 0, 0]) for i in range(n)]
        _enrol_rows(fp, "other", "x", [9 * M], [0])
        before, st0 = fp.neighbour_calls, fp.engine.neighbour_stats()
        got = fp.fp_get_audio_list_neighbours("big", 1, 0.001, -1, -1, 2)
        assert fp.neighbour_calls - before == calls
        assert fp.engine.neighbour_stats()["vote_batches"] - st0["vote_batches"] == calls
        assert [g["uuid"] for g in got] == uu and all(g["frame_count"] == 3 for g in got)
        for g in got:  # every other audio of the context shares the row 9.0; none is itself, none of "other"
            assert len(g["neighbours"]) == min(2, n - 1)
            assert all(x["context"] == "big" and x["uuid"] != g["uuid"] and x["match_count"] >= 1 for x in g["neighbours"])
    finally:
        fp.fp_term()
