"""Host-side mirror of the reference engine facade (/root/reference/src/fp_handler.h:13-38).

Same names, argument meaning and error behaviour as fp_handler.c, so tests read like the
reference's callers (application_handler.c, cli_handler.c, app_tiresias.c):
  * functions return True/False, a dict (the ast_json object) or None (NULL);
  * fp_search_fingerprint_info returns None for both "no match" and "error"
    (fp_handler.c:247-250, :386-390) and otherwise {uuid, name, context, hash,
    frame_count, match_count} (fp_handler.c:394-404);
  * fp_craete_audio_list_info (sic) returns True when the file is already enrolled
    (fp_handler.c:181-185).

The control plane (context_list / audio_list catalog, MD5 dedup, uuid v4) stays on SQLite,
as the reference keeps it; the hot path — fingerprinting and matching — runs on the GPU via
the C-ABI engine. fp_init/fp_term load and write the audio_recongition.db snapshot
(fp_handler.c:68-108) when a backup path is given — catalog tables to SQLite, fingerprint
rows straight into / out of the device index (dbio.py).
"""
from __future__ import annotations

import hashlib
import os
import sqlite3
import uuid as uuidlib
import wave

import numpy as np

from . import dbio
from ._lib import TFP_RANK_MAX, TfpError
from .engine import (ALAW, AUDIO_Q31, AUDIO_S16, AUDIO_ULAW, ULAW, Engine, audio_clips_check, pack_audio_clips, decode_g711, frame_count as frame_count_of, params, read_wav, read_wav_f32,
                     read_wav_g711, read_wav_interleaved, read_wav_interleaved_q31, resample_count, resample_mix_pcm, resample_pcm,
                     resample_wide_pcm)

TFP_E_FORMAT = -8

DEF_SEARCH_TOLERANCE = 0.001  # fp_handler.c:41
DEF_AUBIO_COEFS = 2           # fp_handler.c:39


def read_wav_mono16(filename: str):
    """aubio_source at the file's native rate (DEF_AUBIO_SAMPLERATE 0, fp_handler.c:37, :604):
    int16 PCM + rate, decoded by the engine library (tfp_wav_read). Raises TfpError for a
    missing file (TFP_E_NOENT) or audio the engine cannot take exactly (TFP_E_FORMAT)."""
    return read_wav(filename)


# Headerless Asterisk sound files, told by their extension: G.711 codes, mono at 8 kHz (new
# behaviour: aubio cannot open these, so the reference skips them).
RAW_G711_EXT = {".ulaw": ULAW, ".ul": ULAW, ".mu": ULAW, ".alaw": ALAW, ".al": ALAW}


def read_audio_codes(filename: str):
    """A file as the enrolment takes it: (samples, rate, law). law None: int16 PCM (tfp_wav_read) or,
    failing that, fp32 hop values (tfp_wav_read_f32); law ULAW / ALAW: the uint8 codes of a G.711 WAV
    (tfp_wav_read_g711, tried between the two) or of a headerless .ulaw / .alaw file, for the code
    entry points. Raises TfpError (TFP_E_NOENT, TFP_E_FORMAT)."""
    law = RAW_G711_EXT.get(os.path.splitext(filename)[1].lower())
    if law is not None:
        try:
            with open(filename, "rb") as f:
                return np.frombuffer(f.read(), np.uint8), 8000, law
        except OSError as e:
            raise TfpError(-4, "cannot open %s" % filename) from e
    try:
        return read_wav(filename) + (None,)
    except TfpError as e:
        if e.code != TFP_E_FORMAT:
            raise
    try:
        return read_wav_g711(filename)
    except TfpError as e:
        if e.code != TFP_E_FORMAT:
            raise
    return read_wav_f32(filename) + (None,)


def read_audio(filename: str):
    """aubio_source's mono hop values of a file: int16 PCM (tfp_wav_read) when they are int16 steps
    (8/16-bit mono), the int16 expansion of G.711 codes (a mu-law / A-law WAV, or a headerless
    .ulaw / .alaw file: table[code], expanded on the host), else the fp32 values (tfp_wav_read_f32:
    multichannel mean, 24/32-bit, float). Raises TfpError (TFP_E_NOENT, TFP_E_FORMAT)."""
    x, sr, law = read_audio_codes(filename)
    return (x if law is None else decode_g711(x, law)), sr


def write_wav_mono16(filename: str, pcm: np.ndarray, sample_rate: int = 8000):
    with wave.open(filename, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(np.ascontiguousarray(pcm, "<i2").tobytes())


class FpHandler:
    """One loaded module instance (g_db_ctx + the GPU engine)."""

    def __init__(self, device: int = 0, backup_path: str | None = None, index_rate: int = 0, mix_channels: bool = False,
                 wide_samples: bool = False, mixed_batch: bool = False):
        """backup_path: the snapshot file (the reference hard-codes dbio.DEF_BACKUP_DATABASE);
        None keeps the state in memory only. index_rate: 0 takes every file at its native rate, as the
        reference does (DEF_AUBIO_SAMPLERATE 0); a rate > 0 is the index's rate (new behaviour): int16 and
        G.711 files of another rate are brought to it (tfp_resample_pcm's map: on the GPU in the
        directory enrolment, create_new_audio_info; on the host for a single file, fp_craete_audio_list_info
        and the searches), fp32 files and files at an unsupported rate ratio are refused. mix_channels
        (with an index rate): 8/16-bit integer files of more than one channel at another rate are normalised
        too instead of refused (tfp_resample_mix_pcm's map: the integer downmix, defined for the rate change;
        at the index's own rate such a file keeps the fp32 path, the reference's value). It is off by
        default, so that a handler behaves as it did before the option existed; 24/32-bit and float files
        of another rate are refused either way, unless wide_samples is set. wide_samples (with an index rate;
        off by default for the same reason): a 24/32-bit integer or 32/64-bit float file of another rate is read
        as int32 Q31 frames (tfp_wav_read_interleaved_q31) and normalised by tfp_resample_wide_pcm's map, on
        the GPU in the directory enrolment and on the host for a single file and the searches; several
        channels still need mix_channels. mixed_batch (with an index rate; off by default, so that the
        per-group calls and their counters stay as they were): the directory enrolment hands every file of
        another rate that the options above admit to ONE fingerprint_any_batch (one conversion launch for
        all rates, channel counts and sample kinds; G.711 files go as codes) instead of one call per
        (rate, kind, channels) group. The rows and fingerprints are the same either way."""
        self.device = device
        self.backup_path = backup_path
        self.index_rate = int(index_rate)
        self.mix_channels = bool(mix_channels)
        self.wide_samples = bool(wide_samples)
        self.mixed_batch = bool(mixed_batch)
        self.last_error = ""  # why the last file was refused for its rate
        self.db = None
        self.engine = None
        # context name -> scope id of its clips in the engine (tfp_index_set_scope), from 1 in order of
        # first enrolment: scope 0, a new clip's, belongs to no context
        self._scopes = {}

    def _scope_of(self, context: str, create: bool) -> int:
        """The context's scope id; for a context without clips an id no clip has (create: now its own)."""
        sid = self._scopes.get(context)
        if sid is None:
            sid = len(self._scopes) + 1
            if create:
                self._scopes[context] = sid
        return sid

    # fp_handler.c:68-90 — init_database (the catalog tables) + engine, then the snapshot
    def fp_init(self) -> bool:
        self.db = sqlite3.connect(":memory:", check_same_thread=False)
        dbio.create_catalog(self.db)
        self.engine = Engine(self.device)
        self._scopes = {}
        if self.backup_path:
            try:
                dbio.load_backup(self.db, self.engine, self.backup_path)
                # the loaded clips' scopes from audio_list's context column (one catalog read)
                rows = self.db.execute("select uuid, context from audio_list order by rowid;").fetchall()
                known = [(u, c) for u, c in rows if c is not None and self._indexed(u)]
                if known:
                    self.engine.index_set_scope([u for u, _ in known], [self._scope_of(c, True) for _, c in known])
            except Exception:
                return False  # "Could not load the database data."
        return True

    def _indexed(self, uuid: str) -> bool:
        try:
            self.engine.index_scope(uuid)
        except TfpError:
            return False  # a catalog row without fingerprint rows
        return True

    # fp_handler.c:92-108 — backup, then tear down
    def fp_term(self) -> bool:
        ok = True
        if self.backup_path and self.db and self.engine:
            try:
                dbio.write_backup(self.db, self.engine, self.backup_path)
            except Exception:
                ok = False  # "Could not write database."
        if self.engine:
            self.engine.close()
        self.engine = None
        if self.db:
            self.db.close()
        self.db = None
        return ok

    # ---- contexts (fp_handler.c:912-1095) ----------------------------------------------
    def fp_create_context_list_info(self, name: str, directory: str, replace: bool) -> bool:
        if name is None or directory is None:
            return False
        verb = "insert or replace" if replace else "insert"
        try:
            self.db.execute("%s into context_list(name, directory) values (?, ?);" % verb, (name, directory))
        except sqlite3.Error:
            return False
        return True

    def fp_delete_context_list_info(self, name: str) -> bool:
        if name is None:
            return False
        self.db.execute("delete from context_list where name = ?;", (name,))
        return True

    def fp_get_context_lists_all(self):
        return [dict(zip(("name", "directory"), r)) for r in self.db.execute("select * from context_list;")]

    def fp_get_context_list_info(self, name: str):
        r = self.db.execute("select * from context_list where name = ?;", (name,)).fetchone()
        return dict(zip(("name", "directory"), r)) if r else None

    # ---- audio list ---------------------------------------------------------------------
    def fp_get_audio_lists_all(self):
        return [self._audio_row(r) for r in self.db.execute("select * from audio_list;")]

    def fp_get_audio_lists_by_contextname(self, name: str):
        if name is None:
            return None
        return [self._audio_row(r) for r in self.db.execute("select * from audio_list where context = ?;", (name,))]

    @staticmethod
    def _audio_row(r):
        return dict(zip(("uuid", "name", "context", "hash"), r))

    def _audio_list_info(self, uuid: str):
        r = self.db.execute("select * from audio_list where uuid = ?;", (uuid,)).fetchone()
        return self._audio_row(r) if r else None

    @staticmethod
    def fp_generate_uuid() -> str:
        return str(uuidlib.uuid4())

    @staticmethod
    def fp_create_hash(filename: str):
        try:
            with open(filename, "rb") as f:
                return hashlib.md5(f.read()).hexdigest()
        except OSError:
            return None

    def fp_craete_audio_list_info(self, context: str, filename: str) -> bool:
        """fp_handler.c:161-197: catalog row (MD5 dedup per context) + fingerprint rows."""
        if context is None or filename is None:
            return False
        uuid = self.fp_generate_uuid()
        h = self.fp_create_hash(filename)
        if h is None:
            return False
        if self.db.execute("select * from audio_list where context = ? and hash = ?;", (context, h)).fetchone():
            return True  # already enrolled
        self.db.execute("insert into audio_list(uuid, name, context, hash) values (?, ?, ?, ?);",
                        (uuid, os.path.basename(filename), context, h))
        try:
            pcm, sr = self._read_query(filename)
            fr = self._fingerprint(pcm, [0, len(pcm)], sr)
            self.engine.index_add(uuid, fr["m1"], fr["m2"])
            self.engine.index_set_scope([uuid], [self._scope_of(context, True)])
        except Exception:
            self.fp_delete_audio_list_info(uuid)
            return False
        return True

    # ---- catalog neighbours: which enrolled audios sound like each other (tfp_index_neighbours)
    NEIGHBOUR_FLUSH = 512  # audios per tfp_index_neighbours call

    def _neighbours(self, infos, scope, p, k):
        """infos (catalog rows) with frame_count and neighbours added; an audio the engine does not hold is
        left out. One engine call per NEIGHBOUR_FLUSH audios."""
        infos = [i for i in infos if self._indexed(i["uuid"])]
        out = []
        for a in range(0, len(infos), self.NEIGHBOUR_FLUSH):
            part = infos[a:a + self.NEIGHBOUR_FLUSH]
            res = self.engine.index_neighbours([i["uuid"] for i in part], p, k, [scope] * len(part))
            self.neighbour_calls += 1
            for info, r in zip(part, res):
                info["frame_count"] = r["frame_count"]
                info["neighbours"] = []
                for row in r["neighbours"]:
                    n = self._audio_list_info(row["audio_uuid"])
                    if n is None:
                        continue
                    for key in ("match_count", "aligned_count", "offset", "first_frame", "last_frame"):
                        n[key] = row[key]
                    info["neighbours"].append(n)
                out.append(info)
        return out

    neighbour_calls = 0  # engine calls made by the two entries below (tests)

    def fp_get_audio_list_neighbours(self, context, coefs, tolerance, freq_ignore_low, freq_ignore_high, k):
        """For every audio of the context (fp_get_audio_lists_by_contextname's rows) its catalog fields,
        frame_count (its stored rows) and neighbours: the first k rows of the search of fp_handler.c:287-374
        for its own stored rows over the same context's audios, its own row deleted, each with its catalog
        fields, match_count, aligned_count, offset, first_frame and last_frame."""
        if context is None or coefs < 1 or coefs > DEF_AUBIO_COEFS or k < 1:
            return None
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        return self._neighbours(self.fp_get_audio_lists_by_contextname(context), self._scope_of(context, False), p,
                                min(int(k), TFP_RANK_MAX))

    def fp_get_audio_neighbours(self, uuid, coefs, tolerance, freq_ignore_low, freq_ignore_high, k):
        """The same for one audio, over the audios of every context; None for an unknown uuid."""
        if uuid is None or coefs < 1 or coefs > DEF_AUBIO_COEFS or k < 1:
            return None
        info = self._audio_list_info(uuid)
        if info is None:
            return None
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        got = self._neighbours([info], -1, p, min(int(k), TFP_RANK_MAX))
        return got[0] if got else None

    def _other_rate(self, sr: int) -> bool:
        return self.index_rate > 0 and sr != self.index_rate

    def _refuse_f32(self, filename: str, sr: int) -> str:
        if self.wide_samples:  # what is still missing: the channel option, or a format no reader takes
            why = ("integer PCM of 8 to 32 bits and 32/64-bit float of 1 to 32 channels are taken" if self.mix_channels else
                   "several channels need mix_channels")
            self.last_error = ("%s: fp32 audio at %d Hz cannot be normalised to the index rate %d Hz (%s)"
                               % (filename, sr, self.index_rate, why))
            return self.last_error
        self.last_error = ("%s: fp32 audio at %d Hz cannot be normalised to the index rate %d Hz "
                           "(rate conversion takes 8/16-bit integer PCM and G.711 only%s)"
                           % (filename, sr, self.index_rate, "" if self.mix_channels else ", of several channels with mix_channels"))
        return self.last_error

    def _read_interleaved(self, filename: str):
        """With mix_channels, an fp32 file of another rate as int16[nframes, channels], if it is 8/16-bit
        integer PCM of 1 to 32 channels (tfp_wav_read_interleaved); None for the files that stay refused
        (24/32-bit, float; every fp32 file without mix_channels). With wide_samples, a file the int16 reader
        does not take as int32 Q31 [nframes, channels] (tfp_wav_read_interleaved_q31), several channels only
        with mix_channels; the callers tell the two by the dtype."""
        if self.mix_channels:
            try:
                return read_wav_interleaved(filename)[0]
            except TfpError as e:
                if e.code != TFP_E_FORMAT:
                    raise
        if self.wide_samples:
            try:
                q31 = read_wav_interleaved_q31(filename)[0]
            except TfpError as e:
                if e.code != TFP_E_FORMAT:
                    raise
                return None
            if q31.shape[1] == 1 or self.mix_channels:
                return q31
        return None

    def _read_query(self, filename: str):
        """read_audio for a search: with an index rate set, a file of another rate is normalised on the host
        (G.711 expanded first; an 8/16-bit integer file of several channels by tfp_resample_mix_pcm; with
        wide_samples a 24/32-bit or float file by tfp_resample_wide_pcm); a file none of them takes raises
        TfpError(TFP_E_FORMAT)."""
        pcm, sr = read_audio(filename)
        if not self._other_rate(sr):
            return pcm, sr
        if pcm.dtype == np.float32:
            frames = self._read_interleaved(filename)
            if frames is None:
                raise TfpError(TFP_E_FORMAT, self._refuse_f32(filename, sr))
            convert = resample_wide_pcm if frames.dtype == np.int32 else resample_mix_pcm
            return convert(frames, frames.shape[1], sr, self.index_rate), self.index_rate
        return resample_pcm(pcm, sr, self.index_rate), self.index_rate

    def _fingerprint(self, samples: np.ndarray, offsets, sr: int, law=None, channels: int = 1):
        if self._other_rate(sr):  # (int16: the enrolment expanded G.711 and refused fp32)
            if samples.dtype == np.int32:  # interleaved Q31 frames (wide_samples), offsets in frames
                return self.engine.fingerprint_wide_rate_batch(samples, offsets, channels, sr, self.index_rate)
            if channels > 1:  # interleaved frames, offsets in frames
                return self.engine.fingerprint_mix_rate_batch(samples, offsets, channels, sr, self.index_rate)
            return self.engine.fingerprint_rate_batch(samples, offsets, sr, self.index_rate)
        if law is not None:
            return self.engine.fingerprint_g711_batch(samples, offsets, law, sr)
        if samples.dtype == np.float32:
            return self.engine.fingerprint_f32_batch(samples, offsets, sr)
        return self.engine.fingerprint_batch(samples, offsets, sr)

    def create_new_audio_info(self, context: str) -> bool:
        """app_tiresias.c:365-424 (the module's directory enrolment) batched onto the GPU.

        The reference scans the context's directory (alphasort, without "." and "..") and calls
        fp_craete_audio_list_info per file, skipping files that fail. Here the same catalog rows
        are written in the same order and with the same per-context MD5 dedup (also among the
        files of this scan). The fingerprints of all new files are computed by one fingerprint
        call per sample rate and kind (int16, fp32, G.711 codes of one law, which go to the GPU
        as codes, or with an index rate set interleaved int16 or int32 Q31 of one channel count) and enrolled by one
        tfp_index_add_batch."""
        ctx = self.fp_get_context_list_info(context) if context is not None else None
        if ctx is None or ctx["directory"] is None:
            return False
        directory = ctx["directory"]
        try:
            names = sorted(n for n in os.listdir(directory) if n not in (".", ".."))
        except OSError:
            return False
        new = []  # (uuid, path, pcm, rate)
        seen = set()
        for name in names:
            path = "%s/%s" % (directory, name)
            h = self.fp_create_hash(path)
            if h is None:
                continue  # "Could not create fingerprint info."
            if h in seen or self.db.execute("select * from audio_list where context = ? and hash = ?;",
                                            (context, h)).fetchone():
                continue  # already enrolled
            try:
                pcm, sr, law = read_audio_codes(path)
            except TfpError:
                continue
            channels = 1
            if self._other_rate(sr):
                if law is not None:
                    if not self.mixed_batch:
                        pcm, law = decode_g711(pcm, law), None  # (the converter takes int16)
                elif pcm.dtype == np.float32:
                    try:
                        pcm = self._read_interleaved(path)
                    except TfpError:
                        continue
                    if pcm is None:
                        self._refuse_f32(path, sr)  # refused, as _read_query refuses it for a search
                        continue
                    channels = pcm.shape[1]  # (its frames are counted below: len(pcm))
                if resample_count(len(pcm), sr, self.index_rate) < 0:  # before any catalog row is written
                    self.last_error = "%s: unsupported rate ratio %d -> %d" % (path, sr, self.index_rate)
                    continue
                if self.mixed_batch:  # every rule of the mixed call on this clip alone, before any catalog row is written
                    kind = {np.dtype(np.int16): AUDIO_S16, np.dtype(np.int32): AUDIO_Q31}.get(pcm.dtype, AUDIO_ULAW + (law or 0))
                    try:
                        audio_clips_check([(0, len(pcm), sr, channels, kind, 0)], pcm.nbytes, self.index_rate)
                    except TfpError as e:
                        self.last_error = "%s: %s" % (path, e)
                        continue
            uuid = self.fp_generate_uuid()
            self.db.execute("insert into audio_list(uuid, name, context, hash) values (?, ?, ?, ?);",
                            (uuid, os.path.basename(path), context, h))
            seen.add(h)
            new.append((uuid, pcm, sr, law, channels))
        if self.mixed_batch and self.index_rate > 0:
            # every file of another rate in one call, each clip with its own rate, channel count and kind
            mixed = [n for n in new if self._other_rate(n[2])]
            new = [n for n in new if not self._other_rate(n[2])]
            if mixed:
                data, clips = pack_audio_clips([(n[1], n[2]) if n[3] is None else (n[1], n[2], AUDIO_ULAW + n[3]) for n in mixed])
                fr = self.engine.fingerprint_any_batch(data, clips, self.index_rate)
                lens = audio_clips_check(clips, len(data), self.index_rate)
                foff = np.concatenate([[0], np.cumsum([(int(n) + 255) // 256 for n in lens])]).astype(np.int64)
                self.engine.index_add_batch([n[0] for n in mixed], foff, fr["m1"], fr["m2"])
                self.engine.index_set_scope([n[0] for n in mixed], [self._scope_of(context, True)] * len(mixed))
        for sr, dt, law, channels in sorted({(n[2], n[1].dtype.str, -1 if n[3] is None else n[3], n[4]) for n in new}):
            law = None if law < 0 else law
            group = [n for n in new if n[2] == sr and n[1].dtype.str == dt and n[3] == law and n[4] == channels]
            lens = [len(n[1]) for n in group]  # (frames, for interleaved audio)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            fr = self._fingerprint(np.concatenate([n[1].reshape(-1) for n in group]), off, sr, law, channels)
            if self._other_rate(sr):
                lens = [resample_count(n, sr, self.index_rate) for n in lens]
            foff = np.concatenate([[0], np.cumsum([(n + 255) // 256 for n in lens])]).astype(np.int64)
            self.engine.index_add_batch([n[0] for n in group], foff, fr["m1"], fr["m2"])
            self.engine.index_set_scope([n[0] for n in group], [self._scope_of(context, True)] * len(group))
        return True

    def fp_delete_audio_list_info(self, uuid: str) -> bool:
        """fp_handler.c:115-159: audio_list row + its fingerprint rows."""
        if uuid is None:
            return False
        if self._audio_list_info(uuid) is None:
            return False
        self.db.execute("delete from audio_list where uuid = ?;", (uuid,))
        try:
            self.engine.index_remove(uuid)
        except Exception:
            pass  # no fingerprint rows (e.g. the fingerprint step failed)
        return True

    # ---- search (fp_handler.c:207-408) ------------------------------------------------
    def fp_search_fingerprint_info(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high):
        if context is None or filename is None:
            return None
        if coefs < 1 or coefs > DEF_AUBIO_COEFS:
            return None
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return None
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        if pcm.dtype == np.float32:
            res, _ = self.engine.search_f32_batch(pcm, [0, len(pcm)], p, sr)
        else:
            res, _ = self.engine.search_pcm_batch(pcm, [0, len(pcm)], p, sr)
        hit = res[0]
        if hit is None:
            return None
        info = self._audio_list_info(hit["audio_uuid"])
        if info is None:
            return None
        info["frame_count"] = hit["frame_count"]
        info["match_count"] = hit["match_count"]
        return info

    def fp_search_fingerprint_candidates(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high,
                                         max_results):
        """The first max_results rows of the result query fp_search_fingerprint_info reads one row of
        (fp_handler.c:367-374), each as that call's dict, in rank order; [] where it returns NULL. A
        row whose audio_list entry is missing is skipped (the reference returns NULL for it)."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or max_results < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(max_results), TFP_RANK_MAX)
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
            rows, frame_count = self.engine.search_ranked(fr, p, k), len(fr)
        else:
            rows, frame_count = self.engine.search_ranked_pcm_batch(pcm, [0, len(pcm)], p, k, sr)[0], frame_count_of(len(pcm))
        out = []
        for row in rows:
            info = self._audio_list_info(row["audio_uuid"])
            if info is None:
                continue
            info["frame_count"] = frame_count
            info["match_count"] = row["match_count"]
            out.append(info)
        return out

    def fp_search_fingerprint_in_context(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high,
                                         max_results=1):
        """fp_search_fingerprint_candidates restricted to the clips enrolled in `context`: the search
        the reference documents ("from the context's audio list", doc/dialplan_application.rst:11,
        :52-53) and its per-frame SQL (fp_handler.c:308-314, no context predicate) does not run. The
        rows are the first max_results of fp_handler.c:367-374 over that context's clips alone; [] for a
        context without clips."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or max_results < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(max_results), TFP_RANK_MAX)
        scope = [self._scope_of(context, False)]
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
            rows, frame_count = self.engine.search_scoped_batch(fr, [0, len(fr)], p, scope, k)[0], len(fr)
        else:
            rows = self.engine.search_scoped_pcm_batch(pcm, [0, len(pcm)], p, scope, k, sr)[0]
            frame_count = frame_count_of(len(pcm))
        out = []
        for row in rows:
            info = self._audio_list_info(row["audio_uuid"])
            if info is None:
                continue
            info["frame_count"] = frame_count
            info["match_count"] = row["match_count"]
            out.append(info)
        return out

    def fp_search_fingerprint_census(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high):
        """fp_search_fingerprint_in_context's winner with how it stands against every other clip of
        `context`: the rows of the result query (fp_handler.c:367-374) counted by count(*)
        (tfp_census_batch), which the application's ratio test (application_handler.c:180-203) cannot
        see from the first row. A dict: winner (that call's first row, or None), frame_count,
        population (the context's clips), clips_at_or_above (clips whose count reaches the winner's,
        the winner included), clips_tied (count equal to the winner's) and histogram ([[count, clips],
        ...], non-zero bins only, counts descending). None for bad arguments or an unreadable file."""
        if context is None or filename is None:
            return None
        if coefs < 1 or coefs > DEF_AUBIO_COEFS:
            return None
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return None
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        scope = [self._scope_of(context, False)]
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
            rows, frame_count = self.engine.search_scoped_batch(fr, [0, len(fr)], p, scope, 1)[0], len(fr)
            hist = self.engine.census_batch(fr, [0, len(fr)], p, scope)[0]
        else:
            rows = self.engine.search_scoped_pcm_batch(pcm, [0, len(pcm)], p, scope, 1, sr)[0]
            frame_count = frame_count_of(len(pcm))
            hist = self.engine.census_pcm_batch(pcm, [0, len(pcm)], p, scope, None, sr)[0]
        winner, top = None, 0
        if rows:
            top = rows[0]["match_count"]
            winner = self._audio_list_info(rows[0]["audio_uuid"])
            if winner is not None:
                winner["frame_count"] = frame_count
                winner["match_count"] = top
        return {"winner": winner, "frame_count": frame_count, "population": int(hist.sum()),
                "clips_at_or_above": int(hist[top:].sum()) if top > 0 else 0,
                "clips_tied": int(hist[top]) if top > 0 else 0,
                "histogram": [[c, int(hist[c])] for c in range(len(hist) - 1, -1, -1) if hist[c]]}

    def fp_search_fingerprint_aligned(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high,
                                      max_results):
        """fp_search_fingerprint_candidates' rows, each with where in the clip the recording lies:
        aligned_count (the hits that agree on one time offset), offset (query frame i lies at clip
        frame i + offset), first_frame and last_frame (tfp_alignment). The reference's result query
        (fp_handler.c:367-374) counts the frames that hit; it never reads the rows' frame_idx."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or max_results < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(max_results), TFP_RANK_MAX)
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
            rows, frame_count = self.engine.search_aligned_batch(fr, [0, len(fr)], p, k)[0], len(fr)
        else:
            rows, frame_count = self.engine.search_aligned_pcm_batch(pcm, [0, len(pcm)], p, k, sr)[0], frame_count_of(len(pcm))
        out = []
        for row in rows:
            info = self._audio_list_info(row["audio_uuid"])
            if info is None:
                continue
            info["frame_count"] = frame_count
            for key in ("match_count", "aligned_count", "offset", "first_frame", "last_frame"):
                info[key] = row[key]
            out.append(info)
        return out

    def fp_search_fingerprint_timeline(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high,
                                       window_frames, hop_frames, max_results, in_context=False):
        """fp_search_fingerprint_candidates for every window of a long recording: the reference searches
        one fixed window of audio (application_handler.c:152-185, fp_handler.c:275-374); this returns
        [{"frame": w * hop_frames, "rows": [...]}] for each full window of window_frames frames,
        hop_frames apart, rows being the first max_results rows of fp_handler.c:367-374 over that
        window's frames, each the dict fp_search_fingerprint_candidates builds with frame_count =
        window_frames. in_context restricts every window to the clips enrolled in `context`, as
        fp_search_fingerprint_in_context does. The recording is fingerprinted once. [] for bad arguments
        or a recording shorter than one window."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or max_results < 1 or window_frames < 1 or hop_frames < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(max_results), TFP_RANK_MAX)
        scopes = [self._scope_of(context, False)] if in_context else None
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
            wins = self.engine.search_sliding_batch(fr, [0, len(fr)], p, window_frames, hop_frames, k, scopes)[0]
        else:
            wins = self.engine.search_sliding_pcm_batch(pcm, [0, len(pcm)], p, window_frames, hop_frames, k, scopes, sr)[0]
        out = []
        for w, rows in enumerate(wins):
            infos = []
            for row in rows:
                info = self._audio_list_info(row["audio_uuid"])
                if info is None:
                    continue
                info["frame_count"] = int(window_frames)
                info["match_count"] = row["match_count"]
                infos.append(info)
            out.append({"frame": w * int(hop_frames), "rows": infos})
        return out

    def fp_search_fingerprint_timeline_aligned(self, context, filename, coefs, tolerance, freq_ignore_low,
                                               freq_ignore_high, window_frames, hop_frames, max_results, in_context=False):
        """fp_search_fingerprint_timeline's array, each row also carrying where in the clip its window lies:
        aligned_count, offset, first_frame and last_frame as fp_search_fingerprint_aligned words them
        (window-relative: window frame x lies at clip frame x + offset), and clip_start_frame = frame -
        offset, the recording frame at which clip frame 0 lies, equal across the windows of one
        occurrence of the clip wherever the occurrence's offset alone attains the window's aligned_count (a
        window that fits the clip as well in an earlier place reports that one: the smallest offset wins). The reference's result query (fp_handler.c:367-374) never reads the
        rows' frame_idx. The file is fingerprinted once, then search_sliding_aligned_batch."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or max_results < 1 or window_frames < 1 or hop_frames < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(max_results), TFP_RANK_MAX)
        scopes = [self._scope_of(context, False)] if in_context else None
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
        else:
            fr = self.engine.fingerprint_batch(pcm, [0, len(pcm)], sr)
        wins = self.engine.search_sliding_aligned_batch(fr, [0, len(fr)], p, window_frames, hop_frames, k, scopes)[0]
        out = []
        for w, rows in enumerate(wins):
            infos = []
            for row in rows:
                info = self._audio_list_info(row["audio_uuid"])
                if info is None:
                    continue
                info["frame_count"] = int(window_frames)
                for key in ("match_count", "aligned_count", "offset", "first_frame", "last_frame"):
                    info[key] = row[key]
                info["clip_start_frame"] = w * int(hop_frames) - row["offset"]
                infos.append(info)
            out.append({"frame": w * int(hop_frames), "rows": infos})
        return out

    def fp_search_fingerprint_occurrences(self, context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high,
                                          window_frames, hop_frames, k, max_gap, min_hits):
        """Which clips of `context` play in the recording, and from which frame to which: the join of
        fp_search_fingerprint_timeline_aligned's rows that call leaves to its caller, done by the engine. The
        candidates (clip, clip_start_frame) of the first k rows of every window are each verified along their
        own diagonal over the whole recording with the per-frame predicate of fp_handler.c:287-351, hits at
        most max_gap frames apart forming a segment, and thinned by non-maximum suppression
        (search_occurrences_batch). Returns one dict per occurrence, by first_frame: the clip's audio_list
        row, frame_count (the recording's frames), match_count and hits (those of the segment), clip_start_frame,
        first_frame, last_frame, diagonal_hits, overlap and windows. The context is mapped to a scope as
        fp_search_fingerprint_in_context maps it. [] for bad arguments, a recording shorter than one window or
        a context without clips."""
        if context is None or filename is None:
            return []
        if coefs < 1 or coefs > DEF_AUBIO_COEFS or k < 1 or window_frames < 1 or hop_frames < 1 or max_gap < 0 or min_hits < 1:
            return []
        try:
            pcm, sr = self._read_query(filename)
        except TfpError:
            return []
        p = params(coefs, tolerance, freq_ignore_low, freq_ignore_high)
        k = min(int(k), TFP_RANK_MAX)
        scopes = [self._scope_of(context, False)]
        if pcm.dtype == np.float32:
            fr = self.engine.fingerprint_f32_batch(pcm, [0, len(pcm)], sr)
        else:
            fr = self.engine.fingerprint_batch(pcm, [0, len(pcm)], sr)
        occ = self.engine.search_occurrences_batch(fr, [0, len(fr)], p, window_frames, hop_frames, k, max_gap, min_hits,
                                                   scopes)[0]
        out = []
        for o in occ:
            info = self._audio_list_info(o["audio_uuid"])
            if info is None:
                continue
            info["frame_count"] = len(fr)
            info["match_count"] = o["hits"]
            for key in ("clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap", "windows"):
                info[key] = o[key]
            out.append(info)
        return out

    # ---- live calls: the facade's fp_live_open, fp_live_push and fp_live_occurrences (shim/fp_handler_tfp.h)
    def fp_live_open(self, nchannels: int, sample_rate: int, max_ms: int):
        """A live object of nchannels calls of at most max_ms each (engine.Live), or None for bad arguments."""
        if nchannels <= 0 or sample_rate <= 0 or max_ms <= 0:
            return None
        from .engine import Live
        return Live(self.engine, nchannels, (sample_rate * max_ms + 999) // 1000, sample_rate)

    @staticmethod
    def fp_live_push(lv, slin: np.ndarray, nsamples=None) -> bool:
        """One tick: slin int16[nchannels, tick_samples], channel c taking its first nsamples[c] samples."""
        if lv is None or slin is None:
            return False
        lv.push(slin, None, nsamples=nsamples)
        return True

    def fp_live_occurrences(self, lv, contexts, window_ms, max_gap_ms, min_hits, tolerance, freq_ignore_low,
                            freq_ignore_high, k, sample_rate: int = 8000):
        """The log of each call so far (Live.occurrences): one list per channel, by first_frame, each entry the
        clip's audio_list row with clip_start_frame, first_frame, last_frame, hits, diagonal_hits, overlap and
        windows. window_ms and max_gap_ms convert to frames as tfp_live_window_frames does (0 ms of gap: 0
        frames); coefs is 1, the contexts map to scopes as fp_search_fingerprint_in_context maps them. None for
        bad arguments."""
        if lv is None or contexts is None or window_ms <= 0 or max_gap_ms < 0 or min_hits < 1 or k < 1:
            return None
        if len(contexts) != lv.nchannels or any(c is None for c in contexts):
            return None
        frames = lambda ms: max(1, -(-(ms * sample_rate) // (1000 * 256)))  # noqa: E731  ceil(ms * rate / 1000 / 256)
        p = params(1, tolerance, freq_ignore_low, freq_ignore_high)
        scopes = [self._scope_of(c, False) for c in contexts]
        occ, _ = lv.occurrences(p, scopes, min(int(k), TFP_RANK_MAX), frames(window_ms),
                                frames(max_gap_ms) if max_gap_ms > 0 else 0, min_hits, 64)
        out = []
        for ch in occ:
            rows = []
            for o in ch:
                info = self._audio_list_info(o["audio_uuid"])
                if info is None:
                    continue
                for key in ("clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap", "windows"):
                    info[key] = o[key]
                rows.append(info)
            out.append(rows)
        return out
