"""Pythonic wrapper of the C-ABI engine (numpy in/out)."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from ._lib import Alignment, Candidate, Frame, LiveVerdict, Occurrence, Result, SearchParams, SynthSpec, TfpError, check, lib

FRAME_DTYPE = np.dtype([("frame_idx", "<i4"), ("m1", "<i4"), ("m2", "<i4"), ("reserved", "<i4"),
                        ("q1", "<f8"), ("q2", "<f8")])
assert FRAME_DTYPE.itemsize == C.sizeof(Frame) == 32


def device_count() -> int:
    n = C.c_int32()
    rc = lib().tfp_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def frame_count(nsamples: int) -> int:
    return int(lib().tfp_frame_count(int(nsamples)))


def params(coefs=1, tolerance=-1.0, freq_ignore_low=-1, freq_ignore_high=-1) -> SearchParams:
    return SearchParams(int(coefs), int(freq_ignore_low), int(freq_ignore_high), 0, float(tolerance))


def _wav(call, dtype=np.int16) -> tuple[np.ndarray, int]:
    n, sr = C.c_int64(), C.c_int32()
    check(call(None, 0, C.byref(n), C.byref(sr)))
    pcm = np.empty(n.value, dtype)
    check(call(pcm.ctypes.data, n.value, C.byref(n), C.byref(sr)))
    return pcm, sr.value


def decode_wav(data: bytes) -> tuple[np.ndarray, int]:
    """tfp_wav_decode: RIFF/WAVE bytes -> (mono int16 PCM, native rate), aubio_source semantics
    (fp_handler.c:37, :604, :633). TfpError(TFP_E_FORMAT) for audio the engine cannot take exactly."""
    buf = C.create_string_buffer(bytes(data), len(data))
    return _wav(lambda pcm, cap, n, sr: lib().tfp_wav_decode(buf, len(data), pcm, cap, n, sr))


def read_wav(path: str) -> tuple[np.ndarray, int]:
    """tfp_wav_read: decode_wav of a file."""
    p = path.encode()
    return _wav(lambda pcm, cap, n, sr: lib().tfp_wav_read(p, pcm, cap, n, sr))


def decode_wav_f32(data: bytes) -> tuple[np.ndarray, int]:
    """tfp_wav_decode_f32: RIFF/WAVE bytes -> (fp32 mono hop values as aubio_source computes them,
    native rate), for every PCM width / float format and channel count."""
    buf = C.create_string_buffer(bytes(data), len(data))
    return _wav(lambda x, cap, n, sr: lib().tfp_wav_decode_f32(buf, len(data), x, cap, n, sr), np.float32)


def read_wav_f32(path: str) -> tuple[np.ndarray, int]:
    """tfp_wav_read_f32: decode_wav_f32 of a file."""
    p = path.encode()
    return _wav(lambda x, cap, n, sr: lib().tfp_wav_read_f32(p, x, cap, n, sr), np.float32)


ULAW, ALAW = 0, 1  # TFP_G711_ULAW, TFP_G711_ALAW


def decode_g711(codes, law: int) -> np.ndarray:
    """tfp_g711_decode: G.711 codes -> the int16 aubio_source reads them as (table[code]; exact)."""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    pcm = np.empty(len(codes), np.int16)
    check(lib().tfp_g711_decode(codes.ctypes.data, len(codes), int(law), pcm.ctypes.data))
    return pcm


def resample_count(nsamples: int, rate_in: int, rate_out: int) -> int:
    """tfp_resample_count: the samples nsamples at rate_in become at rate_out (ceil(n L / M)); -1 for a bad
    or unsupported pair."""
    return int(lib().tfp_resample_count(int(nsamples), int(rate_in), int(rate_out)))


def resample_taps(rate_in: int, rate_out: int) -> dict:
    """tfp_resample_taps: {"L", "M", "k_lo", "ntaps", "taps": int16[L, ntaps]}, the pair's Q15 table."""
    v = [C.c_int32() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    check(lib().tfp_resample_taps(int(rate_in), int(rate_out), *refs, None, 0))
    L, ntaps = v[0].value, v[3].value
    taps = np.empty(L * ntaps, np.int16)
    check(lib().tfp_resample_taps(int(rate_in), int(rate_out), *refs, taps.ctypes.data, len(taps)))
    return {"L": L, "M": v[1].value, "k_lo": v[2].value, "ntaps": ntaps, "taps": taps.reshape(L, ntaps)}


def resample_pcm(pcm, rate_in: int, rate_out: int) -> np.ndarray:
    """tfp_resample_pcm: one int16 clip of rate_in at rate_out, the map the GPU rate forms compute (exact)."""
    pcm = np.ascontiguousarray(pcm, np.int16).reshape(-1)
    n = C.c_int64()
    check(lib().tfp_resample_pcm(pcm.ctypes.data, len(pcm), int(rate_in), int(rate_out), None, 0, C.byref(n)))
    out = np.empty(n.value, np.int16)
    check(lib().tfp_resample_pcm(pcm.ctypes.data, len(pcm), int(rate_in), int(rate_out), out.ctypes.data, len(out),
                                 C.byref(n)))
    return out


MIX_CHANNELS_MAX = 32  # TFP_MIX_CHANNELS_MAX


def resample_mix_pcm(pcm, channels: int, rate_in: int, rate_out: int) -> np.ndarray:
    """tfp_resample_mix_pcm: one clip of interleaved int16 frames ([nframes, channels], or flat) downmixed and
    brought to rate_out, the map the GPU mix forms compute (exact)."""
    pcm = np.ascontiguousarray(pcm, np.int16).reshape(-1)
    channels = int(channels)
    nfr = len(pcm) // channels if channels > 0 else 0
    n = C.c_int64()
    check(lib().tfp_resample_mix_pcm(pcm.ctypes.data, nfr, channels, int(rate_in), int(rate_out), None, 0, C.byref(n)))
    out = np.empty(n.value, np.int16)
    check(lib().tfp_resample_mix_pcm(pcm.ctypes.data, nfr, channels, int(rate_in), int(rate_out), out.ctypes.data, len(out),
                                     C.byref(n)))
    return out


def _wav_interleaved(call, dtype=np.int16) -> tuple[np.ndarray, int]:
    n, ch, sr = C.c_int64(), C.c_int32(), C.c_int32()
    check(call(None, 0, C.byref(n), C.byref(ch), C.byref(sr)))
    pcm = np.empty(n.value * ch.value, dtype)
    check(call(pcm.ctypes.data, len(pcm), C.byref(n), C.byref(ch), C.byref(sr)))
    return pcm.reshape(n.value, ch.value), sr.value


def decode_wav_interleaved(data: bytes) -> tuple[np.ndarray, int]:
    """tfp_wav_decode_interleaved: RIFF/WAVE bytes of 8/16-bit integer PCM with 1 to 32 channels ->
    (int16[nframes, channels] as stored, native rate). TfpError(TFP_E_FORMAT) for every other file."""
    buf = C.create_string_buffer(bytes(data), len(data))
    return _wav_interleaved(lambda x, cap, n, ch, sr: lib().tfp_wav_decode_interleaved(buf, len(data), x, cap, n, ch, sr))


def read_wav_interleaved(path: str) -> tuple[np.ndarray, int]:
    """tfp_wav_read_interleaved: decode_wav_interleaved of a file."""
    p = path.encode()
    return _wav_interleaved(lambda x, cap, n, ch, sr: lib().tfp_wav_read_interleaved(p, x, cap, n, ch, sr))


def resample_wide_pcm(q31, channels: int, rate_in: int, rate_out: int) -> np.ndarray:
    """tfp_resample_wide_pcm: one clip of interleaved int32 Q31 frames ([nframes, channels], or flat) downmixed and
    brought to rate_out as int16, the map the GPU wide forms compute (exact)."""
    q31 = np.ascontiguousarray(q31, np.int32).reshape(-1)
    channels = int(channels)
    nfr = len(q31) // channels if channels > 0 else 0
    n = C.c_int64()
    check(lib().tfp_resample_wide_pcm(q31.ctypes.data, nfr, channels, int(rate_in), int(rate_out), None, 0, C.byref(n)))
    out = np.empty(n.value, np.int16)
    check(lib().tfp_resample_wide_pcm(q31.ctypes.data, nfr, channels, int(rate_in), int(rate_out), out.ctypes.data, len(out),
                                      C.byref(n)))
    return out


AUDIO_S16, AUDIO_Q31, AUDIO_ULAW, AUDIO_ALAW = 0, 1, 2, 3  # TFP_AUDIO_*
ANY_RATES_MAX = 64  # TFP_ANY_RATES_MAX
# tfp_audio_clip: a clip of a mixed batch, offset in BYTES into the call's data
CLIP_DTYPE = np.dtype([("offset", "<i8"), ("nframes", "<i8"), ("rate_in", "<i4"), ("channels", "<i4"), ("kind", "<i4"),
                       ("reserved", "<i4")])
_KIND_DTYPE = {AUDIO_S16: np.int16, AUDIO_Q31: np.int32, AUDIO_ULAW: np.uint8, AUDIO_ALAW: np.uint8}


def _any_args(data, clips):
    """(data as contiguous bytes, its size, clips as CLIP_DTYPE records) of a mixed call."""
    data = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    clips = np.ascontiguousarray(clips, CLIP_DTYPE).reshape(-1)
    return data, len(data), clips


def pack_audio_clips(items) -> tuple[np.ndarray, np.ndarray]:
    """The (data, clips) of a mixed batch from (samples, rate_in) or (samples, rate_in, kind) items. samples is
    [nframes, channels] or flat mono; without a kind, int16 samples are AUDIO_S16, int32 AUDIO_Q31 and uint8
    AUDIO_ULAW. Every clip starts at a 4-byte aligned offset."""
    parts, clips, pos = [], np.zeros(len(items), CLIP_DTYPE), 0
    for i, it in enumerate(items):
        x = np.asarray(it[0])
        kind = it[2] if len(it) > 2 else {np.dtype(np.int16): AUDIO_S16, np.dtype(np.int32): AUDIO_Q31,
                                          np.dtype(np.uint8): AUDIO_ULAW}[x.dtype]
        x = np.ascontiguousarray(x, _KIND_DTYPE[kind])
        ch = x.shape[1] if x.ndim == 2 else 1
        raw = x.reshape(-1).view(np.uint8)
        clips[i] = (pos, len(x) if x.ndim == 2 else x.size, int(it[1]), ch, kind, 0)
        pad = -len(raw) % 4
        parts += [raw, np.zeros(pad, np.uint8)]
        pos += len(raw) + pad
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), clips


def audio_clips_check(clips, nbytes: int, rate_out: int) -> np.ndarray:
    """tfp_audio_clips_check: a mixed call's argument rules without an engine; the clips' output lengths at
    rate_out, or TfpError(TFP_E_ARG) naming the first offending clip."""
    clips = np.ascontiguousarray(clips, CLIP_DTYPE).reshape(-1)
    nout = np.zeros(max(len(clips), 1), np.int64)
    check(lib().tfp_audio_clips_check(clips.ctypes.data, len(clips), int(nbytes), int(rate_out), nout.ctypes.data))
    return nout[:len(clips)]


def resample_any_pcm(data, clip, rate_out: int) -> np.ndarray:
    """tfp_resample_any_pcm: one clip of a mixed batch (a CLIP_DTYPE record or its tuple, offset in bytes into
    data) as int16 at rate_out: the existing host map of the clip's class, which the GPU forms compute (exact)."""
    data, nbytes, clip = _any_args(data, clip)
    if len(clip) != 1:
        raise ValueError("one clip")
    # the clip's extent is the caller's to guarantee in the C call: check it here
    need = int(clip["offset"][0]) + int(clip["nframes"][0]) * int(clip["channels"][0]) * \
        np.dtype(_KIND_DTYPE.get(int(clip["kind"][0]), np.uint8)).itemsize
    if int(clip["nframes"][0]) > 0 and int(clip["channels"][0]) > 0 and need > nbytes:
        raise ValueError("the clip reaches past data")
    n = C.c_int64()
    check(lib().tfp_resample_any_pcm(data.ctypes.data, clip.ctypes.data, int(rate_out), None, 0, C.byref(n)))
    out = np.empty(n.value, np.int16)
    check(lib().tfp_resample_any_pcm(data.ctypes.data, clip.ctypes.data, int(rate_out), out.ctypes.data, len(out), C.byref(n)))
    return out


def q31_from_float(x) -> np.ndarray:
    """tfp_q31_from_f32 / tfp_q31_from_f64: float samples (float64 stays double, everything else goes through float32)
    to int32 Q31, rounded to nearest even and clamped; NaN becomes 0."""
    x = np.asarray(x)
    f64 = x.dtype == np.float64
    x = np.ascontiguousarray(x, np.float64 if f64 else np.float32)
    out = np.empty(x.shape, np.int32)
    check((lib().tfp_q31_from_f64 if f64 else lib().tfp_q31_from_f32)(x.ctypes.data, x.size, out.ctypes.data))
    return out


def decode_wav_interleaved_q31(data: bytes) -> tuple[np.ndarray, int]:
    """tfp_wav_decode_interleaved_q31: RIFF/WAVE bytes of 8/16/24/32-bit integer PCM or 32/64-bit float with 1 to 32
    channels -> (int32 Q31 [nframes, channels], native rate). TfpError(TFP_E_FORMAT) for every other file."""
    buf = C.create_string_buffer(bytes(data), len(data))
    return _wav_interleaved(lambda x, cap, n, ch, sr: lib().tfp_wav_decode_interleaved_q31(buf, len(data), x, cap, n, ch, sr),
                            np.int32)


def read_wav_interleaved_q31(path: str) -> tuple[np.ndarray, int]:
    """tfp_wav_read_interleaved_q31: decode_wav_interleaved_q31 of a file."""
    p = path.encode()
    return _wav_interleaved(lambda x, cap, n, ch, sr: lib().tfp_wav_read_interleaved_q31(p, x, cap, n, ch, sr), np.int32)


def _wav_g711(call) -> tuple[np.ndarray, int, int]:
    n, sr, law = C.c_int64(), C.c_int32(), C.c_int32()
    check(call(None, 0, C.byref(n), C.byref(sr), C.byref(law)))
    codes = np.empty(n.value, np.uint8)
    check(call(codes.ctypes.data, n.value, C.byref(n), C.byref(sr), C.byref(law)))
    return codes, sr.value, law.value


def decode_wav_g711(data: bytes) -> tuple[np.ndarray, int, int]:
    """tfp_wav_decode_g711: RIFF/WAVE bytes of a mono mu-law / A-law file -> (codes, native rate, law).
    TfpError(TFP_E_FORMAT) for every other file."""
    buf = C.create_string_buffer(bytes(data), len(data))
    return _wav_g711(lambda c, cap, n, sr, law: lib().tfp_wav_decode_g711(buf, len(data), c, cap, n, sr, law))


def read_wav_g711(path: str) -> tuple[np.ndarray, int, int]:
    """tfp_wav_read_g711: decode_wav_g711 of a file."""
    p = path.encode()
    return _wav_g711(lambda c, cap, n, sr, law: lib().tfp_wav_read_g711(p, c, cap, n, sr, law))


def synth_specs(seed: int, clips, offsets=None):
    clips = list(clips)
    offsets = [0] * len(clips) if offsets is None else list(offsets)
    arr = (SynthSpec * max(1, len(clips)))()
    for i, (c, o) in enumerate(zip(clips, offsets)):
        arr[i] = SynthSpec(seed & (2**64 - 1), int(c), int(o))
    return arr


def synth_pcm(seed: int, clips, samples_per_clip: int, offsets=None) -> np.ndarray:
    """Deterministic synthetic PCM (host side of tfp_synth_pcm) -> int16[nclips, samples]."""
    clips = list(clips)
    out = np.zeros((len(clips), samples_per_clip), np.int16)
    specs = synth_specs(seed, clips, offsets)
    check(lib().tfp_synth_pcm(specs, len(clips), samples_per_clip, out.ctypes.data))
    return out


TRACE_KEYS = ("overlap", "hits", "segments", "seg_hits", "seg_first", "seg_last")


def sliding_windows(nframes: int, window: int, hop: int) -> int:
    """tfp_sliding_windows: full windows of `window` frames, `hop` apart, in a recording of nframes frames."""
    return int(lib().tfp_sliding_windows(int(nframes), int(window), int(hop)))


class _SlidingCalls:
    """Sliding search, the same calls on an Engine (tfp_*) and on a Group (tfp_group_*), as _ScopedCalls."""

    def _sliding(self, name, data, offsets, nframes, head, p, window, hop, scopes, k, aligned=False):
        nrec, k = len(offsets) - 1, int(k)
        if scopes is not None:
            scopes = np.ascontiguousarray(scopes, np.int32)
            if len(scopes) != nrec:
                raise ValueError("one scope per recording")
        per = [sliding_windows(n, window, hop) for n in nframes]
        cap, nw = sum(per), C.c_int64()
        out, counts = (Candidate * max(1, cap * max(k, 1)))(), (C.c_int32 * max(1, cap))()
        align = ((Alignment * max(1, cap * max(k, 1)))(),) if aligned else ()
        self._chk(self._fn(name)(self._h, data.ctypes.data, offsets.ctypes.data, nrec, *head, C.byref(p), int(window),
                                 int(hop), None if scopes is None else scopes.ctypes.data, k, out, counts, *align, cap,
                                 C.byref(nw)))
        assert nw.value == cap
        rows = Engine._aligned(out, align[0], counts, cap, k) if aligned else Engine._candidates(out, counts, cap, k)
        woff = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        return [rows[woff[r]:woff[r + 1]] for r in range(nrec)]

    def search_sliding_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, window: int, hop: int, k: int,
                             scopes=None):
        """tfp_search_sliding_batch: per recording a list over its windows (window w = frames [w * hop, w * hop +
        window) of the recording) of the rows search_scoped_batch gives for that window's frames with the
        recording's scope (None: every clip)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        return self._sliding("_search_sliding_batch", frames, qoffsets, np.diff(qoffsets), (), p, window, hop, scopes, k)

    def search_sliding_pcm_batch(self, pcm, offsets, p: SearchParams, window: int, hop: int, k: int, scopes=None,
                                 sample_rate: int = 8000):
        """tfp_search_sliding_pcm_batch: search_sliding_batch over each recording's own fingerprint."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        return self._sliding("_search_sliding_pcm_batch", pcm, offsets, [frame_count(n) for n in np.diff(offsets)],
                             (int(sample_rate),), p, window, hop, scopes, k)


    def search_sliding_aligned_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, window: int, hop: int, k: int,
                                     scopes=None):
        """tfp_search_sliding_aligned_batch: search_sliding_batch's rows, each with the alignment (aligned_count,
        offset, first_frame, last_frame, window-relative) of its window's frames with its clip. The rows of one
        occurrence of a clip share w * hop - offset across windows wherever that offset alone attains the count."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        return self._sliding("_search_sliding_aligned_batch", frames, qoffsets, np.diff(qoffsets), (), p, window, hop,
                             scopes, k, aligned=True)

    # ---- occurrence search: which clips play in a recording, from which frame to which
    OCCURRENCE_KEYS = ("recording", "clip_id", "clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits",
                       "overlap", "windows")

    def _occurrences(self, name, data, offsets, head, p, window, hop, scopes, k, max_gap, min_hits):
        nrec = len(offsets) - 1
        if scopes is not None:
            scopes = np.ascontiguousarray(scopes, np.int32)
            if len(scopes) != nrec:
                raise ValueError("one scope per recording")
        args = (self._h, data.ctypes.data, offsets.ctypes.data, nrec, *head, C.byref(p), int(window), int(hop),
                None if scopes is None else scopes.ctypes.data, int(k), int(max_gap), int(min_hits))
        n, cap = C.c_int64(), 1024
        while True:  # (TFP_E_CAPACITY names the room the list needs)
            out = (Occurrence * cap)()
            rc = self._fn(name)(*args, out, cap, C.byref(n))
            if rc != -5 or n.value <= cap:
                break
            cap = n.value
        self._chk(rc)
        per = [[] for _ in range(nrec)]
        for o in out[:n.value]:
            row = {"audio_uuid": o.uuid.decode()}
            row.update({f: getattr(o, f) for f in self.OCCURRENCE_KEYS})
            per[o.recording].append(row)
        return per

    def search_occurrences_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, window: int, hop: int, k: int,
                                 max_gap: int, min_hits: int, scopes=None):
        """tfp_search_occurrences_batch: per recording the list of occurrence dicts (audio_uuid, clip_start_frame,
        first_frame, last_frame, hits, diagonal_hits, overlap, windows, clip_id, recording), by first_frame: the
        candidates (clip, w * hop - offset) of search_sliding_aligned_batch's rows, each traced along its own
        diagonal over the whole recording and thinned by non-maximum suppression."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        return self._occurrences("_search_occurrences_batch", frames, qoffsets, (), p, window, hop, scopes, k, max_gap,
                                 min_hits)


class _ScopedCalls:
    """Scoped search, the same calls on an Engine (tfp_*) and on a Group (tfp_group_*): _PFX names which."""

    def _fn(self, name):
        return getattr(lib(), self._PFX + name)

    def index_set_scope(self, uuids, scopes):
        """tfp_index_set_scope: clip uuids[i] gets scope scopes[i] (>= 0); all or nothing."""
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != len(uuids):
            raise ValueError("one scope per uuid")
        arr = (C.c_char_p * max(1, len(uuids)))(*[u.encode() for u in uuids])
        self._chk(self._fn("_index_set_scope")(self._h, len(uuids), arr, scopes.ctypes.data))

    def index_scope(self, uuid: str) -> int:
        s = C.c_int32()
        self._chk(self._fn("_index_scope")(self._h, uuid.encode(), C.byref(s)))
        return s.value

    def search_scoped_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, scopes, k: int):
        """search_ranked_batch with query q restricted to the clips of scopes[q] (TFP_SCOPE_ANY: every clip)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != nq:
            raise ValueError("one scope per query")
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(self._fn("_search_scoped_batch")(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p),
                                                   scopes.ctypes.data, k, out, counts))
        return Engine._candidates(out, counts, nq, k)

    def search_scoped_pcm_batch(self, pcm, offsets, p: SearchParams, scopes, k: int, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != nq:
            raise ValueError("one scope per query")
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(self._fn("_search_scoped_pcm_batch")(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                       C.byref(p), scopes.ctypes.data, k, out, counts))
        return Engine._candidates(out, counts, nq, k)

    def index_neighbours(self, uuids, p: SearchParams, k: int, scopes=None, aligned: bool = True):
        """tfp_index_neighbours: per named clip {"frame_count", "neighbours"}: the first k rows of the result
        query for the clip's own stored rows over the clips of scopes[i] (None: every clip), its own row
        deleted; with aligned each row carries its alignment's four fields."""
        n, k = len(uuids), int(k)
        arr = (C.c_char_p * max(1, n))(*[u.encode() for u in uuids])
        sp = None
        if scopes is not None:
            scopes = np.ascontiguousarray(scopes, np.int32)
            if len(scopes) != n:
                raise ValueError("one scope per uuid")
            sp = scopes.ctypes.data
        m = max(1, n * max(k, 1))
        out, counts, fc = (Candidate * m)(), (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
        align = (Alignment * m)() if aligned else None
        self._chk(self._fn("_index_neighbours")(self._h, n, arr, C.byref(p), sp, k, out, align, counts, fc))
        rows = Engine._aligned(out, align, counts, n, k) if aligned else Engine._candidates(out, counts, n, k)
        return [{"frame_count": fc[i], "neighbours": rows[i]} for i in range(n)]


def census_at_least(hist_row, count: int) -> int:
    """tfp_census_at_least: the clips of one census row with count >= `count` (bin 0 only for count <= 0)."""
    row = np.ascontiguousarray(hist_row, np.int32)
    return int(lib().tfp_census_at_least(row.ctypes.data, len(row), int(count)))


class _RateCalls:
    """Rate-normalised ingest, the same calls on an Engine (tfp_*) and on a Group (tfp_group_*), as _ScopedCalls:
    int16 clips of rate_in converted to rate_out on the GPU in front of the unchanged fingerprint kernels."""

    resample_count = staticmethod(resample_count)
    resample_taps = staticmethod(resample_taps)
    resample_pcm = staticmethod(resample_pcm)

    def fingerprint_rate_batch(self, pcm, offsets, rate_in: int, rate_out: int) -> np.ndarray:
        """The frames of fingerprint_batch(resample_pcm(clip), rate_out) per clip, bit for bit."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(max(resample_count(int(offsets[i + 1] - offsets[i]), rate_in, rate_out), 0))
                for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(self._fn("_fingerprint_rate_batch")(self._h, pcm.ctypes.data, offsets.ctypes.data, nclips, int(rate_in),
                                                      int(rate_out), out.ctypes.data, n, C.byref(got)))
        return out[:got.value]

    def search_rate_batch(self, pcm, offsets, rate_in: int, rate_out: int, p: SearchParams):
        """search_pcm_batch at rate_out on the resampled queries."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(self._fn("_search_rate_batch")(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, int(rate_in),
                                                 int(rate_out), C.byref(p), res))
        return Engine._results(res, nq)

    def search_scoped_rate_batch(self, pcm, offsets, rate_in: int, rate_out: int, p: SearchParams, scopes, k: int):
        """search_scoped_pcm_batch at rate_out on the resampled queries: (rows per query, frame counts)."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != nq:
            raise ValueError("one scope per query")
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        fc = (C.c_int32 * max(1, nq))()
        self._chk(self._fn("_search_scoped_rate_batch")(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, int(rate_in),
                                                        int(rate_out), C.byref(p), scopes.ctypes.data, k, out, counts, fc))
        return Engine._candidates(out, counts, nq, k), list(fc[:nq])


class _MixCalls:
    """Rate-normalised ingest of multichannel int16, the same calls on an Engine and on a Group, as _RateCalls:
    pcm holds interleaved frames of `channels` int16 each and offsets count frames."""

    resample_mix_pcm = staticmethod(resample_mix_pcm)

    @staticmethod
    def _mix_count(nframes: int, rate_in: int, rate_out: int) -> int:
        return int(nframes) if rate_in == rate_out else max(resample_count(nframes, rate_in, rate_out), 0)

    def fingerprint_mix_rate_batch(self, pcm, offsets, channels: int, rate_in: int, rate_out: int) -> np.ndarray:
        """The frames of fingerprint_batch(resample_mix_pcm(clip), rate_out) per clip, bit for bit."""
        return self._frames_fingerprint("mix", np.int16, pcm, offsets, channels, rate_in, rate_out)

    def search_mix_rate_batch(self, pcm, offsets, channels: int, rate_in: int, rate_out: int, p: SearchParams):
        """search_pcm_batch at rate_out on the downmixed, resampled queries."""
        return self._frames_search("mix", np.int16, pcm, offsets, channels, rate_in, rate_out, p)

    def search_scoped_mix_rate_batch(self, pcm, offsets, channels: int, rate_in: int, rate_out: int, p: SearchParams, scopes,
                                     k: int):
        """search_scoped_pcm_batch at rate_out on the downmixed, resampled queries: (rows per query, frame counts)."""
        return self._frames_search_scoped("mix", np.int16, pcm, offsets, channels, rate_in, rate_out, p, scopes, k)

    # the bodies, shared with the wide forms (_WideCalls): kind names the entry point, dtype the samples
    def _frames_fingerprint(self, kind: str, dtype, pcm, offsets, channels: int, rate_in: int, rate_out: int) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(self._mix_count(int(offsets[i + 1] - offsets[i]), rate_in, rate_out)) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(self._fn("_fingerprint_%s_rate_batch" % kind)(self._h, pcm.ctypes.data, offsets.ctypes.data, nclips, int(channels),
                                                          int(rate_in), int(rate_out), out.ctypes.data, n, C.byref(got)))
        return out[:got.value]

    def _frames_search(self, kind: str, dtype, pcm, offsets, channels: int, rate_in: int, rate_out: int, p: SearchParams):
        pcm = np.ascontiguousarray(pcm, dtype)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(self._fn("_search_%s_rate_batch" % kind)(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, int(channels),
                                                     int(rate_in), int(rate_out), C.byref(p), res))
        return Engine._results(res, nq)

    def _frames_search_scoped(self, kind: str, dtype, pcm, offsets, channels: int, rate_in: int, rate_out: int,
                              p: SearchParams, scopes, k: int):
        pcm = np.ascontiguousarray(pcm, dtype)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != nq:
            raise ValueError("one scope per query")
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        fc = (C.c_int32 * max(1, nq))()
        self._chk(self._fn("_search_scoped_%s_rate_batch" % kind)(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, int(channels),
                                                            int(rate_in), int(rate_out), C.byref(p), scopes.ctypes.data, k, out,
                                                            counts, fc))
        return Engine._candidates(out, counts, nq, k), list(fc[:nq])


class _WideCalls:
    """Rate-normalised ingest of 24/32-bit and float audio, the same calls on an Engine and on a Group: q31 holds
    interleaved frames of `channels` int32 Q31 each and offsets count frames (the bodies are _MixCalls')."""

    resample_wide_pcm = staticmethod(resample_wide_pcm)

    def fingerprint_wide_rate_batch(self, q31, offsets, channels: int, rate_in: int, rate_out: int) -> np.ndarray:
        """The frames of fingerprint_batch(resample_wide_pcm(clip), rate_out) per clip, bit for bit."""
        return self._frames_fingerprint("wide", np.int32, q31, offsets, channels, rate_in, rate_out)

    def search_wide_rate_batch(self, q31, offsets, channels: int, rate_in: int, rate_out: int, p: SearchParams):
        """search_pcm_batch at rate_out on the converted queries."""
        return self._frames_search("wide", np.int32, q31, offsets, channels, rate_in, rate_out, p)

    def search_scoped_wide_rate_batch(self, q31, offsets, channels: int, rate_in: int, rate_out: int, p: SearchParams, scopes,
                                      k: int):
        """search_scoped_pcm_batch at rate_out on the converted queries: (rows per query, frame counts)."""
        return self._frames_search_scoped("wide", np.int32, q31, offsets, channels, rate_in, rate_out, p, scopes, k)


class _AnyCalls:
    """Mixed batches, the same calls on an Engine and on a Group: data holds the call's bytes and clips its
    tfp_audio_clip records (CLIP_DTYPE, or tuples in its order; pack_audio_clips builds both)."""

    resample_any_pcm = staticmethod(resample_any_pcm)

    def fingerprint_any_batch(self, data, clips, rate_out: int) -> np.ndarray:
        """The frames of fingerprint_batch(resample_any_pcm(clip), rate_out) per clip, bit for bit; one conversion launch."""
        data, nbytes, clips = _any_args(data, clips)
        nout = np.zeros(max(len(clips), 1), np.int64)
        # the host check sizes the output; a call it refuses goes on to the engine, whose refusal is the one raised
        ok = lib().tfp_audio_clips_check(clips.ctypes.data, len(clips), nbytes, int(rate_out), nout.ctypes.data) == 0
        n = sum(frame_count(int(x)) for x in nout[:len(clips)]) if ok else 0
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(self._fn("_fingerprint_any_batch")(self._h, data.ctypes.data, nbytes, clips.ctypes.data, len(clips),
                                                     int(rate_out), out.ctypes.data, n, C.byref(got)))
        return out[:got.value]

    def search_any_batch(self, data, clips, rate_out: int, p: SearchParams):
        """search_pcm_batch at rate_out on the converted queries."""
        data, nbytes, clips = _any_args(data, clips)
        nq = len(clips)
        res = (Result * max(1, nq))()
        self._chk(self._fn("_search_any_batch")(self._h, data.ctypes.data, nbytes, clips.ctypes.data, nq, int(rate_out),
                                                C.byref(p), res))
        return Engine._results(res, nq)

    def search_scoped_any_batch(self, data, clips, rate_out: int, p: SearchParams, scopes, k: int):
        """search_scoped_pcm_batch at rate_out on the converted queries: (rows per query, frame counts)."""
        data, nbytes, clips = _any_args(data, clips)
        nq, k = len(clips), int(k)
        scopes = np.ascontiguousarray(scopes, np.int32)
        if len(scopes) != nq:
            raise ValueError("one scope per query")
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        fc = (C.c_int32 * max(1, nq))()
        self._chk(self._fn("_search_scoped_any_batch")(self._h, data.ctypes.data, nbytes, clips.ctypes.data, nq, int(rate_out),
                                                       C.byref(p), scopes.ctypes.data, k, out, counts, fc))
        return Engine._candidates(out, counts, nq, k), list(fc[:nq])


class _CensusCalls:
    """The match census, the same calls on an Engine (tfp_*) and on a Group (tfp_group_*), as _ScopedCalls."""

    def _census(self, name, data, offsets, nframes, head, p, scopes, nbins):
        nq = len(offsets) - 1
        if scopes is not None:
            scopes = np.ascontiguousarray(scopes, np.int32)
            if len(scopes) != nq:
                raise ValueError("one scope per query")
        if nbins is None:
            nbins = max([int(n) for n in nframes], default=0) + 1
        hist = np.zeros((nq, int(nbins)), np.int32)
        need = C.c_int32()
        self._chk(self._fn(name)(self._h, data.ctypes.data, offsets.ctypes.data, nq, *head, C.byref(p),
                                 None if scopes is None else scopes.ctypes.data, int(nbins), hist.ctypes.data,
                                 C.byref(need)))
        return hist

    def census_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, scopes=None, nbins=None) -> np.ndarray:
        """tfp_census_batch: int32[nq, nbins], hist[q, c] = the live clips of scopes[q] (None: every clip)
        whose count for query q is c, as search_scoped_batch would report it were k unbounded; bin 0
        holds the scope's clips with no hit. nbins None: the longest query's frames + 1."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        return self._census("_census_batch", frames, qoffsets, np.diff(qoffsets), (), p, scopes, nbins)

    def census_pcm_batch(self, pcm, offsets, p: SearchParams, scopes=None, nbins=None, sample_rate: int = 8000) -> np.ndarray:
        """tfp_census_pcm_batch: census_batch of the recordings' frames, fingerprinted on the device."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        return self._census("_census_pcm_batch", pcm, offsets, [frame_count(int(n)) for n in np.diff(offsets)],
                            (int(sample_rate),), p, scopes, nbins)


class Engine(_ScopedCalls, _SlidingCalls, _CensusCalls, _RateCalls, _MixCalls, _WideCalls, _AnyCalls):
    """One engine per GPU (tfp_engine)."""
    _PFX = "tfp"

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        rc = lib().tfp_engine_create(int(device), C.byref(self._h))
        if rc != 0:
            raise TfpError(rc, f"cannot create engine on device {device}")
        self.device = device
        self._streams = weakref.WeakSet()  # live Streams: destroyed before the engine (tiresias_fp.h)

    def close(self):
        if self._h:
            for st in list(self._streams):
                st.close()
            lib().tfp_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def _chk(self, rc):
        return check(rc, self._h)

    def last_error(self) -> str:
        """tfp_engine_last_error for the calling thread ("" when no call has failed)."""
        return (lib().tfp_engine_last_error(self._h) or b"").decode()

    # ---- fingerprinting -----------------------------------------------------------
    def fingerprint(self, pcm: np.ndarray, sample_rate: int = 8000) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, np.int16)
        n = frame_count(len(pcm))
        out = np.zeros(n, FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_fingerprint_pcm(self._h, pcm.ctypes.data, len(pcm), sample_rate, out.ctypes.data, n,
                                            C.byref(got)))
        return out

    def fingerprint_batch(self, pcm: np.ndarray, offsets, sample_rate: int = 8000) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(int(offsets[i + 1] - offsets[i])) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_fingerprint_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nclips, sample_rate,
                                              out.ctypes.data, n, C.byref(got)))
        return out[:n]

    def fingerprint_f32_batch(self, x: np.ndarray, offsets, sample_rate: int = 8000) -> np.ndarray:
        """tfp_fingerprint_f32_batch: fingerprint_batch over fp32 hop values (decode_wav_f32)."""
        x = np.ascontiguousarray(x, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(int(offsets[i + 1] - offsets[i])) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_fingerprint_f32_batch(self._h, x.ctypes.data, offsets.ctypes.data, nclips, sample_rate,
                                                  out.ctypes.data, n, C.byref(got)))
        return out[:n]

    def fingerprint_g711_batch(self, codes: np.ndarray, offsets, law: int, sample_rate: int = 8000) -> np.ndarray:
        """tfp_fingerprint_g711_batch: fingerprint_batch over G.711 codes, expanded on the GPU; the
        frames equal fingerprint_batch(decode_g711(codes, law)) bit for bit."""
        codes = np.ascontiguousarray(codes, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(int(offsets[i + 1] - offsets[i])) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_fingerprint_g711_batch(self._h, codes.ctypes.data, offsets.ctypes.data, nclips, int(law),
                                                   sample_rate, out.ctypes.data, n, C.byref(got)))
        return out[:n]

    def g711_stats(self) -> dict:
        """tfp_g711_stats: batch expansion launches, code stream ticks and the codes they took."""
        v = [C.c_int64() for _ in range(3)]
        self._chk(lib().tfp_g711_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("expand_launches", "stream_launches", "codes"), (x.value for x in v)))

    def resample_stats(self) -> dict:
        """tfp_resample_stats: rate conversion launches, the samples they read and the samples they wrote."""
        v = [C.c_int64() for _ in range(3)]
        self._chk(lib().tfp_resample_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "samples_in", "samples_out"), (x.value for x in v)))

    def resample_mix_stats(self) -> dict:
        """tfp_resample_mix_stats: the multichannel kernel's launches, the frames they read, the samples they
        wrote, and how many of the launches staged their channel sums in LDS."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(lib().tfp_resample_mix_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "frames_in", "samples_out", "staged_launches"), (x.value for x in v)))

    def resample_wide_stats(self) -> dict:
        """tfp_resample_wide_stats: the wide kernel's launches, the frames they read, the samples they wrote, and
        how many of the launches staged in LDS."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(lib().tfp_resample_wide_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "frames_in", "samples_out", "staged_launches"), (x.value for x in v)))

    _ANY_STATS = ("launches", "clips", "frames_in", "samples_out", "tiles_staged", "tiles_global", "tiles_plain")

    def resample_any_stats(self) -> dict:
        """tfp_resample_any_stats: the mixed kernel's launches, the clips and frames they read, the samples they
        wrote, and their tiles by form (staged in LDS, per-tap in global memory, plain at equal rates)."""
        v = [C.c_int64() for _ in range(7)]
        self._chk(lib().tfp_resample_any_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(Engine._ANY_STATS, (x.value for x in v)))

    def fingerprint_stats(self) -> dict:
        """tfp_fingerprint_stats: fingerprint kernel launches so far, by kernel."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(lib().tfp_fingerprint_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("small8k", "throughput8k", "generic_i16", "generic_f32"), (x.value for x in v)))

    # ---- index ----------------------------------------------------------------------
    def index_add(self, uuid: str, m1, m2) -> int:
        m1 = np.ascontiguousarray(m1, np.int32)
        m2 = np.ascontiguousarray(m2, np.int32)
        cid = C.c_int32()
        self._chk(lib().tfp_index_add(self._h, uuid.encode(), m1.ctypes.data, m2.ctypes.data, len(m1), C.byref(cid)))
        return cid.value

    def index_add_batch(self, uuids, frame_offsets, m1, m2):
        frame_offsets = np.ascontiguousarray(frame_offsets, np.int64)
        m1 = np.ascontiguousarray(m1, np.int32)
        m2 = np.ascontiguousarray(m2, np.int32)
        arr = (C.c_char_p * max(1, len(uuids)))(*[u.encode() for u in uuids])
        self._chk(lib().tfp_index_add_batch(self._h, len(uuids), arr, frame_offsets.ctypes.data, m1.ctypes.data,
                                            m2.ctypes.data))

    def index_rows(self, uuid: str):
        """Stored (m1, m2) micro-unit rows of one clip, frame order."""
        n = C.c_int64()
        rc = lib().tfp_index_rows(self._h, uuid.encode(), None, None, 0, C.byref(n))
        if rc not in (0, -5):
            self._chk(rc)
        m1 = np.zeros(max(n.value, 1), np.int32)
        m2 = np.zeros(max(n.value, 1), np.int32)
        self._chk(lib().tfp_index_rows(self._h, uuid.encode(), m1.ctypes.data, m2.ctypes.data, n.value, C.byref(n)))
        return m1[:n.value], m2[:n.value]

    def index_remove(self, uuid: str):
        self._chk(lib().tfp_index_remove(self._h, uuid.encode()))

    def index_clear(self):
        self._chk(lib().tfp_index_clear(self._h))

    def index_stats(self):
        r, c = C.c_int64(), C.c_int32()
        self._chk(lib().tfp_index_stats(self._h, C.byref(r), C.byref(c)))
        return r.value, c.value

    def index_commit(self):
        self._chk(lib().tfp_index_commit(self._h))

    def index_build_stats(self):
        """(full builds, incremental merges) of the sorted index so far."""
        f, m = C.c_int64(), C.c_int64()
        self._chk(lib().tfp_index_build_stats(self._h, C.byref(f), C.byref(m)))
        return f.value, m.value

    def index_delta_stats(self):
        """(delta updates so far, clips in the index delta now)."""
        u, c = C.c_int64(), C.c_int32()
        self._chk(lib().tfp_index_delta_stats(self._h, C.byref(u), C.byref(c)))
        return u.value, c.value

    def sweep_stats(self) -> dict:
        """The coefs = 2 sweep's sort path per batch (tfp_sweep_stats): bin sort, library sort,
        redone speculative passes, crowd bins copied."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(lib().tfp_sweep_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("bins", "library", "redone", "crowd"), [x.value for x in v]))

    def search_path_stats(self) -> dict:
        """tfp_search_path_stats: the plain-search batches each form served so far."""
        v = [C.c_int64() for _ in range(5)]
        self._chk(lib().tfp_search_path_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("small", "vote_class", "vote_gemm", "vote_redone", "general"), (x.value for x in v)))

    def index_cache_stats(self) -> dict:
        """The coefs = 2 clip-set caches (tfp_index_cache_stats): builds, cached hits, builds from the
        clip order, the clip order's full builds and merges, the index delta's caches and sweeps."""
        v = [C.c_int64() for _ in range(7)]
        self._chk(lib().tfp_index_cache_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("builds", "hits", "from_order", "order_builds", "order_merges", "delta_builds", "delta_sweeps"),
                        [x.value for x in v]))

    def set_tiebreak(self, keys):
        keys = np.ascontiguousarray(keys, np.int32)
        self._chk(lib().tfp_index_set_tiebreak(self._h, keys.ctypes.data, len(keys)))

    def update_tiebreak(self, first_clip_id: int, keys):
        """tfp_index_update_tiebreak: the override's keys of clip ids first_clip_id.. only."""
        keys = np.ascontiguousarray(keys, np.int32)
        self._chk(lib().tfp_index_update_tiebreak(self._h, int(first_clip_id), keys.ctypes.data, len(keys)))

    def uuid_of_key(self, key: int) -> str:
        buf = C.create_string_buffer(64)
        self._chk(lib().tfp_index_uuid_of_key(self._h, int(key), buf, 64))
        return buf.value.decode()

    # ---- search ---------------------------------------------------------------------
    @staticmethod
    def _results(res, n):
        return [None if not r.found else {"audio_uuid": r.uuid.decode(), "match_count": r.match_count,
                                          "frame_count": r.frame_count, "clip_id": r.clip_id}
                for r in res[:n]], [r.frame_count for r in res[:n]]

    def search_batch(self, frames: np.ndarray, qoffsets, p: SearchParams):
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq = len(qoffsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_search_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p), res))
        return self._results(res, nq)

    def search(self, frames: np.ndarray, p: SearchParams):
        r, fc = self.search_batch(frames, [0, len(frames)], p)
        return r[0], fc[0]

    def search_pcm_batch(self, pcm: np.ndarray, offsets, p: SearchParams, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_search_pcm_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                             C.byref(p), res))
        return self._results(res, nq)

    def search_g711_batch(self, codes: np.ndarray, offsets, law: int, p: SearchParams, sample_rate: int = 8000):
        """tfp_search_g711_batch: search_pcm_batch over G.711 codes, expanded on the GPU."""
        codes = np.ascontiguousarray(codes, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_search_g711_batch(self._h, codes.ctypes.data, offsets.ctypes.data, nq, int(law), sample_rate,
                                              C.byref(p), res))
        return self._results(res, nq)

    def search_f32_batch(self, x: np.ndarray, offsets, p: SearchParams, sample_rate: int = 8000):
        """tfp_search_f32_batch: search_pcm_batch over fp32 hop values."""
        x = np.ascontiguousarray(x, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_search_f32_batch(self._h, x.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                             C.byref(p), res))
        return self._results(res, nq)

    # ---- ranked search: per query the first k rows of the reference's result set, in rank order
    @staticmethod
    def _candidates(out, counts, nq, k):
        return [[{"audio_uuid": c.uuid.decode(), "match_count": c.match_count, "clip_id": c.clip_id}
                 for c in out[q * k:q * k + counts[q]]] for q in range(nq)]

    def search_ranked_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, k: int):
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_search_ranked_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p), k,
                                                out, counts))
        return self._candidates(out, counts, nq, k)

    def search_ranked(self, frames: np.ndarray, p: SearchParams, k: int):
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        k = int(k)
        out, count = (Candidate * max(1, k))(), C.c_int32()
        self._chk(lib().tfp_search_ranked(self._h, frames.ctypes.data, len(frames), C.byref(p), k, out, C.byref(count)))
        return self._candidates(out, [count.value], 1, k)[0]

    def search_ranked_pcm_batch(self, pcm: np.ndarray, offsets, p: SearchParams, k: int, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_search_ranked_pcm_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                    C.byref(p), k, out, counts))
        return self._candidates(out, counts, nq, k)

    # ---- aligned search: where in each candidate clip the query matches (tfp_alignment)
    @staticmethod
    def _alignment(a):
        return {"aligned_count": a.aligned_count, "offset": a.offset, "first_frame": a.first_frame,
                "last_frame": a.last_frame}

    @staticmethod
    def _aligned(out, align, counts, nq, k):
        """The ranked rows, each with its alignment's four fields."""
        rows = Engine._candidates(out, counts, nq, k)
        for q in range(nq):
            for r, row in enumerate(rows[q]):
                row.update(Engine._alignment(align[q * k + r]))
        return rows

    def align_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, clip_ids, k: int):
        """tfp_align_batch: per query k alignment dicts, query q against clip_ids[q * k + r] (-1: a zeroed row)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        ids = np.ascontiguousarray(clip_ids, np.int32).reshape(-1)
        if len(ids) != nq * max(k, 0):
            raise ValueError("clip_ids must hold nqueries * k ids")
        out = (Alignment * max(1, nq * max(k, 1)))()
        self._chk(lib().tfp_align_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p),
                                        ids.ctypes.data, k, out))
        return [[self._alignment(out[q * k + r]) for r in range(k)] for q in range(nq)]

    def search_aligned_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, k: int):
        """search_ranked_batch's rows, each with aligned_count, offset, first_frame, last_frame."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        n = max(1, nq * max(k, 1))
        out, align, counts = (Candidate * n)(), (Alignment * n)(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_search_aligned_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p), k,
                                                 out, align, counts))
        return self._aligned(out, align, counts, nq, k)

    def search_aligned_pcm_batch(self, pcm: np.ndarray, offsets, p: SearchParams, k: int, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        n = max(1, nq * max(k, 1))
        out, align, counts = (Candidate * n)(), (Alignment * n)(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_search_aligned_pcm_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                     C.byref(p), k, out, align, counts))
        return self._aligned(out, align, counts, nq, k)

    def align_stats(self) -> dict:
        """tfp_align_stats: batches that reached the alignment kernels and the pairs they named."""
        b, n = C.c_int64(), C.c_int64()
        self._chk(lib().tfp_align_stats(self._h, C.byref(b), C.byref(n)))
        return {"batches": b.value, "pairs": n.value}

    # ---- sliding aligned search: each window's rows with where the clip lies
    def align_sliding_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, window: int, hop: int, clip_ids, k: int):
        """tfp_align_sliding_batch: per recording a list over its windows of k alignment dicts, window j (numbered
        over all recordings) against clip_ids[j * k + i] (-1: a zeroed row)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nrec, k = len(qoffsets) - 1, int(k)
        per = [sliding_windows(n, window, hop) for n in np.diff(qoffsets)]
        cap, nw = sum(per), C.c_int64()
        ids = np.ascontiguousarray(clip_ids, np.int32).reshape(-1)
        if len(ids) != cap * max(k, 0):
            raise ValueError("clip_ids must hold nwindows * k ids")
        out = (Alignment * max(1, cap * max(k, 1)))()
        self._chk(lib().tfp_align_sliding_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nrec, C.byref(p),
                                                int(window), int(hop), ids.ctypes.data, k, out, cap, C.byref(nw)))
        assert nw.value == cap
        woff = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        return [[[self._alignment(out[j * k + i]) for i in range(k)] for j in range(woff[r], woff[r + 1])]
                for r in range(nrec)]

    def search_sliding_aligned_pcm_batch(self, pcm, offsets, p: SearchParams, window: int, hop: int, k: int, scopes=None,
                                         sample_rate: int = 8000):
        """tfp_search_sliding_aligned_pcm_batch: search_sliding_aligned_batch over each recording's own fingerprint."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        return self._sliding("_search_sliding_aligned_pcm_batch", pcm, offsets, [frame_count(n) for n in np.diff(offsets)],
                             (int(sample_rate),), p, window, hop, scopes, k, aligned=True)

    # ---- diagonal trace and occurrence search
    def trace_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, reqs, max_gap: int):
        """tfp_trace_batch: reqs = [(recording, clip_id, start), ...]; per request a dict (overlap, hits, segments,
        seg_hits, seg_first, seg_last) of the clip laid on the recording with its frame 0 at recording frame start."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        r = np.zeros((len(reqs), 4), np.int32)
        if len(reqs):
            r[:, :3] = np.asarray(reqs, np.int64).reshape(-1, 3)
        out = np.zeros((max(1, len(reqs)), 6), np.int32)
        self._chk(lib().tfp_trace_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, len(qoffsets) - 1, C.byref(p),
                                        r.ctypes.data, len(reqs), int(max_gap), out.ctypes.data))
        return [dict(zip(TRACE_KEYS, map(int, row))) for row in out[:len(reqs)]]

    def search_occurrences_pcm_batch(self, pcm, offsets, p: SearchParams, window: int, hop: int, k: int, max_gap: int,
                                     min_hits: int, scopes=None, sample_rate: int = 8000):
        """tfp_search_occurrences_pcm_batch: search_occurrences_batch over each recording's own fingerprint."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        return self._occurrences("_search_occurrences_pcm_batch", pcm, offsets, (int(sample_rate),), p, window, hop, scopes,
                                 k, max_gap, min_hits)

    def trace_stats(self) -> dict:
        """tfp_trace_stats: batches that launched the trace kernel, and the requests it computed."""
        b, n = C.c_int64(), C.c_int64()
        self._chk(lib().tfp_trace_stats(self._h, C.byref(b), C.byref(n)))
        return {"batches": b.value, "traces": n.value}

    def slide_align_stats(self) -> dict:
        """tfp_slide_align_stats: batches that reached the sliding alignment, and the entries aligned by form."""
        b, s, d = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(lib().tfp_slide_align_stats(self._h, C.byref(b), C.byref(s), C.byref(d)))
        return {"batches": b.value, "slid_entries": s.value, "direct_entries": d.value}

    def rank_stats(self) -> dict:
        """tfp_rank_stats: ranked batches served by the vote form and by the general form."""
        v, g = C.c_int64(), C.c_int64()
        self._chk(lib().tfp_rank_stats(self._h, C.byref(v), C.byref(g)))
        return {"vote_batches": v.value, "general_batches": g.value}

    def scope_stats(self) -> dict:
        """tfp_scope_stats: scoped batches by form, and builds of the per-column scope table."""
        v, g, t = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(lib().tfp_scope_stats(self._h, C.byref(v), C.byref(g), C.byref(t)))
        return {"vote_batches": v.value, "general_batches": g.value, "table_builds": t.value}

    def neighbour_stats(self) -> dict:
        """tfp_neighbour_stats: neighbour calls by form, the rows aligned, the stored rows used as query frames."""
        x = [C.c_int64() for _ in range(4)]
        self._chk(lib().tfp_neighbour_stats(self._h, *[C.byref(v) for v in x]))
        return dict(zip(("vote_batches", "general_batches", "pairs_aligned", "frames_read"), (v.value for v in x)))

    def census_stats(self) -> dict:
        """tfp_census_stats: census batches served by the vote form and by the general form."""
        v, g = C.c_int64(), C.c_int64()
        self._chk(lib().tfp_census_stats(self._h, C.byref(v), C.byref(g)))
        return {"vote_batches": v.value, "general_batches": g.value}

    def slide_stats(self) -> dict:
        """tfp_slide_stats: sliding batches by form, and the windows they held."""
        v, g, w = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(lib().tfp_slide_stats(self._h, C.byref(v), C.byref(g), C.byref(w)))
        return {"vote_batches": v.value, "general_batches": g.value, "windows": w.value}

    # ---- device-resident paths (pointers are raw device addresses, e.g. tensor.data_ptr())
    def plan(self, offsets, sample_rate: int = 8000) -> "Plan":
        return Plan(self, offsets, sample_rate)

    def fingerprint_device(self, plan: "Plan", d_pcm: int, d_micro: int, d_db: int = 0, stream: int = 0):
        self._chk(lib().tfp_fingerprint_device(self._h, plan.handle, C.c_void_p(d_pcm), C.c_void_p(d_micro),
                                               C.c_void_p(d_db or None), C.c_void_p(stream or None)))

    def index_add_device(self, uuids, frame_offsets, d_micro: int, stream: int = 0):
        frame_offsets = np.ascontiguousarray(frame_offsets, np.int64)
        arr = (C.c_char_p * max(1, len(uuids)))(*[u.encode() for u in uuids])
        self._chk(lib().tfp_index_add_device(self._h, len(uuids), arr, frame_offsets.ctypes.data,
                                             C.c_void_p(d_micro), C.c_void_p(stream or None)))

    def search_device(self, plan: "Plan", d_pcm: int, p: SearchParams, d_keys: int, stream: int = 0):
        self._chk(lib().tfp_search_device(self._h, plan.handle, C.c_void_p(d_pcm), C.byref(p), C.c_void_p(d_keys),
                                          C.c_void_p(stream or None)))

    def search_q_device(self, d_q: int, qoffsets, p: SearchParams, d_keys: int, stream: int = 0):
        """tfp_search_q_device: search from device-resident frame values (2 doubles per frame)."""
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        self._chk(lib().tfp_search_q_device(self._h, C.c_void_p(d_q), qoffsets.ctypes.data, len(qoffsets) - 1,
                                            C.byref(p), C.c_void_p(d_keys), C.c_void_p(stream or None)))

    def synth_device(self, seed: int, clips, samples_per_clip: int, d_out: int, offsets=None, stream: int = 0):
        clips = list(clips)
        specs = synth_specs(seed, clips, offsets)
        self._chk(lib().tfp_synth_pcm_device(self._h, specs, len(clips), samples_per_clip, C.c_void_p(d_out),
                                             C.c_void_p(stream or None)))

    def synchronize(self, stream: int = 0):
        self._chk(lib().tfp_synchronize(self._h, C.c_void_p(stream or None)))


class Stream:
    """Live channels (tfp_stream): rolling window fingerprint + match per tick."""

    def __init__(self, eng: Engine, nchannels: int, window_samples: int, sample_rate: int = 8000):
        self._eng = eng
        self._h = C.c_void_p()
        eng._chk(lib().tfp_stream_create(eng.handle, int(nchannels), int(sample_rate), int(window_samples),
                                         C.byref(self._h)))
        self.nchannels = nchannels
        self.window_samples = int(window_samples)
        self._res = (Result * nchannels)()
        eng._streams.add(self)

    def reset(self, channel: int = -1):
        self._eng._chk(lib().tfp_stream_reset(self._h, int(channel)))

    def push(self, pcm: np.ndarray, p: SearchParams = None):
        """pcm int16[nchannels, tick] -> list of per-channel results (None = NOTFOUND / not full)."""
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.shape[0] == self.nchannels
        self._eng._chk(lib().tfp_stream_push(self._h, pcm.ctypes.data, pcm.shape[1],
                                             C.byref(p) if p is not None else None, self._res if p is not None else None))
        if p is None:
            return None
        return [None if not r.found else {"audio_uuid": r.uuid.decode(), "match_count": r.match_count,
                                          "frame_count": r.frame_count} for r in self._res]

    def push_g711(self, codes: np.ndarray, law: int, p: SearchParams = None):
        """codes uint8[nchannels, tick] of one law -> as push (the scatter into the ring expands them)."""
        codes = np.ascontiguousarray(codes, np.uint8)
        assert codes.shape[0] == self.nchannels
        self._eng._chk(lib().tfp_stream_push_g711(self._h, codes.ctypes.data, codes.shape[1], int(law),
                                                  C.byref(p) if p is not None else None,
                                                  self._res if p is not None else None))
        if p is None:
            return None
        return [None if not r.found else {"audio_uuid": r.uuid.decode(), "match_count": r.match_count,
                                          "frame_count": r.frame_count} for r in self._res]

    def window_frames(self, channel: int) -> np.ndarray:
        """tfp_stream_window_frames: the frames of the channel's current window (0 frames until it is full)."""
        n = frame_count(self.window_samples)
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._eng._chk(lib().tfp_stream_window_frames(self._h, int(channel), out.ctypes.data, n, C.byref(got)))
        return out[:got.value]

    def close(self):
        # tfp_stream_destroy uses the engine: a stream outliving its engine's close() was already
        # destroyed by it, so there is nothing left to free here
        if self._h and self._eng._h:
            lib().tfp_stream_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LiveCalls:
    """Live calls (tfp_live / tfp_group_live): the same calls on an Engine's and on a Group's object."""

    def _open(self, owner, nchannels: int, max_samples: int, sample_rate: int, rate_in=None):
        self._owner = owner
        self._h = C.c_void_p()
        if rate_in is None:
            rc = self._fn("_create")(owner.handle, int(nchannels), int(sample_rate), int(max_samples), C.byref(self._h))
        else:
            rc = self._fn("_create_rate")(owner.handle, int(nchannels), int(rate_in), int(sample_rate), int(max_samples),
                                          C.byref(self._h))
        owner._chk(rc)
        self.nchannels = int(nchannels)
        self.max_samples = int(max_samples)
        owner._streams.add(self)

    def _fn(self, name):
        return getattr(lib(), self._PFX + name)

    def reset(self, channel: int = -1):
        """A new call on `channel` (< 0: every channel) starts empty."""
        self._owner._chk(self._fn("_reset")(self._h, int(channel)))

    def samples(self, channel: int) -> int:
        n = C.c_int64()
        self._owner._chk(self._fn("_samples")(self._h, int(channel), C.byref(n)))
        return n.value

    def input_samples(self, channel: int) -> int:
        """tfp_live_input_samples: the input samples the channel has taken since its last reset (at rate_in)."""
        n = C.c_int64()
        self._owner._chk(self._fn("_input_samples")(self._h, int(channel), C.byref(n)))
        return n.value

    def rate_info(self) -> dict:
        """tfp_live_rate_info: rate_in and lag_in (k_hi input samples; 0 on a plain object)."""
        r, lag = C.c_int32(), C.c_int64()
        self._owner._chk(self._fn("_rate_info")(self._h, C.byref(r), C.byref(lag)))
        return {"rate_in": r.value, "lag_in": lag.value}

    def _rate_stats(self, *lead):
        v = [C.c_int64() for _ in range(3)]
        self._owner._chk(self._fn("_rate_stats")(self._h, *lead, *[C.byref(x) for x in v]))
        return dict(zip(("launches", "samples_in", "samples_out"), (x.value for x in v)))

    def finish(self, channels=None):
        """The end of a call on a rate object: lag_in int16 zeros to the named channels (None: every channel),
        ingest only, after which every output of their calls is settled. Nothing on a plain object."""
        lag = self.rate_info()["lag_in"]
        if lag <= 0:
            return
        ns = np.zeros(self.nchannels, np.int32)
        ns[list(range(self.nchannels)) if channels is None else list(channels)] = lag
        self.push(np.zeros((self.nchannels, lag), np.int16), nsamples=ns)

    def push(self, pcm: np.ndarray, p: SearchParams = None, scopes=None, k: int = 1, nsamples=None):
        """pcm int16[nchannels, tick]; channel c takes its first nsamples[c] samples (None: the whole tick).
        p None: ingest only, returns None. Else (rows, frame_counts): per channel the first k rows of the
        scoped search of its call so far (scopes None: TFP_SCOPE_ANY) and its frame count."""
        return self._push(np.ascontiguousarray(pcm, np.int16), None, p, scopes, k, nsamples)

    def push_g711(self, codes: np.ndarray, law: int, p: SearchParams = None, scopes=None, k: int = 1, nsamples=None):
        """push over G.711 codes uint8[nchannels, tick] of TFP_G711_ULAW / TFP_G711_ALAW: the results of
        push(g711_decode(codes, law), ...), the codes expanded on the GPU."""
        return self._push(np.ascontiguousarray(codes, np.uint8), int(law), p, scopes, k, nsamples)

    def _push(self, tick, law, p, scopes, k, nsamples):
        assert tick.ndim == 2 and tick.shape[0] == self.nchannels
        n, k = self.nchannels, int(k)
        ns = None if nsamples is None else np.ascontiguousarray(nsamples, np.int32)
        sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
        if (ns is not None and len(ns) != n) or (sc is not None and len(sc) != n):
            raise ValueError("one entry per channel")
        out, counts, fc = (Candidate * max(1, n * max(k, 1)))(), (C.c_int32 * n)(), (C.c_int32 * n)()
        rest = (None if ns is None else ns.ctypes.data, C.byref(p) if p is not None else None,
                None if sc is None else sc.ctypes.data, k, out, counts, fc)
        if law is None:
            rc = self._fn("_push")(self._h, tick.ctypes.data, tick.shape[1], *rest)
        else:
            rc = self._fn("_push_g711")(self._h, tick.ctypes.data, tick.shape[1], law, *rest)
        self._owner._chk(rc)
        if p is None:
            return None
        return Engine._candidates(out, counts, n, k), list(fc)

    def verdict(self, total_samples, p: SearchParams, scopes=None):
        """tfp_live_verdict: per channel a dict of leader / rival ({"audio_uuid", "match_count", "clip_id"} or
        None), remaining, complete and decided, for calls planned to reach total_samples[c] samples."""
        n = self.nchannels
        tot = np.ascontiguousarray(total_samples, np.int64)
        sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
        if len(tot) != n or (sc is not None and len(sc) != n):
            raise ValueError("one entry per channel")
        out = (LiveVerdict * n)()
        self._owner._chk(self._fn("_verdict")(self._h, tot.ctypes.data, C.byref(p) if p is not None else None,
                                              None if sc is None else sc.ctypes.data, out))

        def cand(c, has):
            return {"audio_uuid": c.uuid.decode(), "match_count": c.match_count, "clip_id": c.clip_id} if has else None
        return [{"leader": cand(v.leader, v.has_leader), "rival": cand(v.rival, v.has_rival), "remaining": v.remaining,
                 "complete": bool(v.complete), "decided": bool(v.decided)} for v in out]

    def window(self, p: SearchParams, scopes=None, k: int = 1, window: int = 1):
        """tfp_live_window: (rows, frame_counts, first_frames), per channel the first k rows of the scoped
        search of the last `window` frames of its call so far (the tail included), how many frames that
        is and the first of them. Ingests nothing."""
        n, k = self.nchannels, int(k)
        sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
        if sc is not None and len(sc) != n:
            raise ValueError("one entry per channel")
        out, counts = (Candidate * max(1, n * max(k, 1)))(), (C.c_int32 * n)()
        fc, ff = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._owner._chk(self._fn("_window")(self._h, C.byref(p) if p is not None else None,
                                             None if sc is None else sc.ctypes.data, k, int(window), out, counts, fc, ff))
        return Engine._candidates(out, counts, n, k), list(fc), list(ff)

    def window_aligned(self, p: SearchParams, scopes=None, k: int = 1, window: int = 1):
        """tfp_live_window_aligned: (rows, aligns, frame_counts, first_frames): window()'s rows, frame counts
        and first frames, and per channel k alignment dicts (aligned_count, offset, first_frame, last_frame,
        relative to the window; zeros past the channel's rows). Clip frame 0 of row r of channel c lies at
        call frame first_frames[c] - aligns[c][r]["offset"]. Ingests nothing."""
        n, k = self.nchannels, int(k)
        sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
        if sc is not None and len(sc) != n:
            raise ValueError("one entry per channel")
        m = max(1, n * max(k, 1))
        out, align, counts = (Candidate * m)(), (Alignment * m)(), (C.c_int32 * n)()
        fc, ff = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._owner._chk(self._fn("_window_aligned")(self._h, C.byref(p) if p is not None else None,
                                                     None if sc is None else sc.ctypes.data, k, int(window), out, align,
                                                     counts, fc, ff))
        aligns = [[Engine._alignment(align[c * k + r]) for r in range(k)] for c in range(n)]
        return Engine._candidates(out, counts, n, k), aligns, list(fc), list(ff)

    def occurrences(self, p: SearchParams, scopes=None, k: int = 1, window: int = 1, max_gap: int = 0, min_hits: int = 1,
                    max_tracks: int = 64, cap: int = None):
        """tfp_live_occurrences: (occurrences, dropped): per channel the occurrence dicts of its call so far
        (audio_uuid, clip_start_frame, first_frame, last_frame, hits, diagonal_hits, overlap, windows, clip_id,
        recording = the channel), by first_frame, and per channel the candidates this call's offer dropped.
        Ingests nothing. cap: the capacity handed to the call (None: grown to what it needs)."""
        n = self.nchannels
        sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
        if sc is not None and len(sc) != n:
            raise ValueError("one entry per channel")
        dropped, got = (C.c_int32 * n)(), C.c_int64()
        room = n * 64 if cap is None else int(cap)  # (TFP_LIVE_TRACKS_MAX per channel: every track an occurrence)
        out = (Occurrence * max(room, 1))()
        self._owner._chk(self._fn("_occurrences")(self._h, C.byref(p) if p is not None else None,
                                                  None if sc is None else sc.ctypes.data, int(k), int(window), int(max_gap),
                                                  int(min_hits), int(max_tracks), out, room, C.byref(got), dropped))
        per = [[] for _ in range(n)]
        for o in out[:got.value]:
            row = {"audio_uuid": o.uuid.decode()}
            row.update({f: getattr(o, f) for f in _SlidingCalls.OCCURRENCE_KEYS})
            per[o.recording].append(row)
        return per, list(dropped)

    def tracks(self, channel: int):
        """tfp_live_tracks: the channel's list as of the last occurrences() call, in list order: dicts of
        clip_id, start (s), reserved, windows and the trace's fields (overlap, hits, segments, seg_hits,
        seg_first, seg_last)."""
        cap, got = 64, C.c_int64()
        reqs, tr, win = np.zeros((cap, 4), np.int32), np.zeros((cap, 6), np.int32), np.zeros(cap, np.int32)
        self._owner._chk(self._fn("_tracks")(self._h, int(channel), reqs.ctypes.data, tr.ctypes.data, win.ctypes.data, cap,
                                             C.byref(got)))
        return [dict(clip_id=int(reqs[i, 1]), start=int(reqs[i, 2]), reserved=int(reqs[i, 3]), windows=int(win[i]),
                     **dict(zip(TRACE_KEYS, map(int, tr[i])))) for i in range(got.value)]

    def _occurrence_stats(self, *lead):
        v = [C.c_int64() for _ in range(5)]
        self._owner._chk(self._fn("_occurrence_stats")(self._h, *lead, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "tracks_added", "tracks_dropped", "frames_traced", "retraces"), (x.value for x in v)))

    def _window_aligned_stats(self, *lead):
        v = [C.c_int64() for _ in range(3)]
        self._owner._chk(self._fn("_window_aligned_stats")(self._h, *lead, *[C.byref(x) for x in v]))
        return dict(zip(("inplace_calls", "general_calls", "pairs"), (x.value for x in v)))

    def frames(self, channel: int, first: int = 0, cap: int = None) -> np.ndarray:
        """tfp_live_frames: the kept frames [first, F) of the channel's call so far (exact q values).
        cap: the capacity handed to the call (None: what it needs)."""
        got = C.c_int64()
        if cap is None:
            cap = max(frame_count(self.samples(channel)) - int(first), 0)
        out = np.zeros(max(int(cap), 1), FRAME_DTYPE)
        self._owner._chk(self._fn("_frames")(self._h, int(channel), int(first), out.ctypes.data, int(cap), C.byref(got)))
        return out[:got.value]

    def _window_stats(self, *lead):
        v = [C.c_int64() for _ in range(6)]
        self._owner._chk(self._fn("_window_stats")(self._h, *lead, *[C.byref(x) for x in v]))
        return dict(zip(("slid_calls", "general_calls", "rebuilds", "frames_added", "frames_removed", "rows_restarted"),
                        (x.value for x in v)))

    def close(self):
        # the destroy call uses the owner: an object outliving its owner's close() was destroyed by it
        if self._h and self._owner._h:
            self._fn("_destroy")(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Live(_LiveCalls):
    """tfp_live: every channel's call so far on one engine, the per-clip counts carried from push to push."""
    _PFX = "tfp_live"

    def __init__(self, eng: Engine, nchannels: int, max_samples: int, sample_rate: int = 8000, rate_in: int = None):
        """rate_in: the rate the ticks arrive at (tfp_live_create_rate); None: sample_rate, a plain object.
        max_samples and everything returned are at sample_rate."""
        self._open(eng, nchannels, max_samples, sample_rate, rate_in)

    def rate_stats(self) -> dict:
        """tfp_live_rate_stats: conversion launches of this object's pushes, input samples taken, samples settled."""
        return self._rate_stats()

    def stats(self) -> dict:
        """tfp_live_stats: searching pushes by form, count-table rebuilds, frames fingerprinted and added."""
        v = [C.c_int64() for _ in range(5)]
        self._owner._chk(lib().tfp_live_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("incremental_pushes", "general_pushes", "rebuilds", "frames_fingerprinted", "frames_added"),
                        (x.value for x in v)))

    def window_stats(self) -> dict:
        """tfp_live_window_stats: window calls by form, table restarts, frames added and removed, rows restarted."""
        return self._window_stats()

    def window_aligned_stats(self) -> dict:
        """tfp_live_window_aligned_stats: aligned window calls by form, and the pairs given to the alignment kernels."""
        return self._window_aligned_stats()

    def occurrence_stats(self) -> dict:
        """tfp_live_occurrence_stats: occurrence calls, tracks added and dropped, (track, frame) pairs folded, retraces."""
        return self._occurrence_stats()


class Plan:
    def __init__(self, eng: Engine, offsets, sample_rate: int = 8000):
        offsets = np.ascontiguousarray(offsets, np.int64)
        self._h = C.c_void_p()
        eng._chk(lib().tfp_plan_create(eng.handle, offsets.ctypes.data, len(offsets) - 1, sample_rate,
                                       C.byref(self._h)))
        self.nframes = int(lib().tfp_plan_frames(self._h))
        self.offsets = offsets

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if self._h:
            lib().tfp_plan_destroy(self._h)
            self._h = C.c_void_p()


class Group(_ScopedCalls, _SlidingCalls, _CensusCalls, _RateCalls, _MixCalls, _WideCalls, _AnyCalls):
    """tfp_group: one engine per listed device (a device may repeat), the enrolled clips sharded
    over them, searches combined on the host (tiresias_fp.h, device groups)."""
    _PFX = "tfp_group"

    def __init__(self, devices):
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        rc = lib().tfp_group_create(devs, len(devices), C.byref(self._h))
        if rc != 0:
            raise TfpError(rc, f"cannot create a group on devices {list(devices)}")
        self.devices = list(devices)
        self._streams = weakref.WeakSet()

    def close(self):
        if self._h:
            for st in list(self._streams):
                st.close()
            lib().tfp_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _chk(self, rc):
        if rc != 0:
            raise TfpError(rc, lib().tfp_group_last_error(self._h).decode())
        return rc

    def size(self) -> int:
        return int(lib().tfp_group_size(self._h))

    def tiebreak_stats(self) -> dict:
        """tfp_group_tiebreak_stats: key respaces, new-clip-only pushes, shard delta updates that
        re-sent every main column's key."""
        v = [C.c_int64() for _ in range(3)]
        check(lib().tfp_group_tiebreak_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("respaces", "partial_pushes", "shard_full_key_updates"), [x.value for x in v]))

    def peer_stats(self) -> dict:
        """Peer access among the group's distinct devices (tfp_group_peer_stats): ordered pairs,
        how many may access each other, for how many it is enabled."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().tfp_group_peer_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"pairs": a.value, "can_access": b.value, "enabled": c.value}

    def engine_stats(self):
        """[(rows, clips)] of every shard's engine."""
        out = []
        for s in range(self.size()):
            r, c = C.c_int64(), C.c_int32()
            check(lib().tfp_index_stats(lib().tfp_group_engine(self._h, s), C.byref(r), C.byref(c)))
            out.append((r.value, c.value))
        return out

    def fingerprint_batch(self, pcm, offsets, sample_rate: int = 8000) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(int(offsets[i + 1] - offsets[i])) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_group_fingerprint_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nclips, sample_rate,
                                                    out.ctypes.data, n, C.byref(got)))
        return out[:n]

    def resample_stats(self) -> dict:
        """tfp_resample_stats summed over the shards' engines."""
        tot = {"launches": 0, "samples_in": 0, "samples_out": 0}
        for sh in range(self.size()):
            v = [C.c_int64() for _ in range(3)]
            check(lib().tfp_resample_stats(lib().tfp_group_engine(self._h, sh), *[C.byref(x) for x in v]))
            for key, x in zip(tot, v):
                tot[key] += x.value
        return tot

    def resample_mix_stats(self) -> list:
        """tfp_resample_mix_stats of every shard's engine, in shard order."""
        keys, out = ("launches", "frames_in", "samples_out", "staged_launches"), []
        for sh in range(self.size()):
            v = [C.c_int64() for _ in range(4)]
            check(lib().tfp_resample_mix_stats(lib().tfp_group_engine(self._h, sh), *[C.byref(x) for x in v]))
            out.append(dict(zip(keys, (x.value for x in v))))
        return out

    def resample_wide_stats(self) -> list:
        """tfp_resample_wide_stats of every shard's engine, in shard order."""
        keys, out = ("launches", "frames_in", "samples_out", "staged_launches"), []
        for sh in range(self.size()):
            v = [C.c_int64() for _ in range(4)]
            check(lib().tfp_resample_wide_stats(lib().tfp_group_engine(self._h, sh), *[C.byref(x) for x in v]))
            out.append(dict(zip(keys, (x.value for x in v))))
        return out

    def resample_any_stats(self) -> list:
        """tfp_resample_any_stats of every shard's engine, in shard order."""
        out = []
        for sh in range(self.size()):
            v = [C.c_int64() for _ in range(7)]
            check(lib().tfp_resample_any_stats(lib().tfp_group_engine(self._h, sh), *[C.byref(x) for x in v]))
            out.append(dict(zip(Engine._ANY_STATS, (x.value for x in v))))
        return out

    def fingerprint_g711_batch(self, codes, offsets, law: int, sample_rate: int = 8000) -> np.ndarray:
        codes = np.ascontiguousarray(codes, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nclips = len(offsets) - 1
        n = sum(frame_count(int(offsets[i + 1] - offsets[i])) for i in range(nclips))
        out = np.zeros(max(n, 1), FRAME_DTYPE)
        got = C.c_int64()
        self._chk(lib().tfp_group_fingerprint_g711_batch(self._h, codes.ctypes.data, offsets.ctypes.data, nclips, int(law),
                                                         sample_rate, out.ctypes.data, n, C.byref(got)))
        return out[:n]

    def index_add(self, uuid: str, m1, m2):
        m1 = np.ascontiguousarray(m1, np.int32)
        m2 = np.ascontiguousarray(m2, np.int32)
        self._chk(lib().tfp_group_index_add(self._h, uuid.encode(), m1.ctypes.data, m2.ctypes.data, len(m1)))

    def index_add_batch(self, uuids, frame_offsets, m1, m2):
        frame_offsets = np.ascontiguousarray(frame_offsets, np.int64)
        m1 = np.ascontiguousarray(m1, np.int32)
        m2 = np.ascontiguousarray(m2, np.int32)
        arr = (C.c_char_p * max(1, len(uuids)))(*[u.encode() for u in uuids])
        self._chk(lib().tfp_group_index_add_batch(self._h, len(uuids), arr, frame_offsets.ctypes.data, m1.ctypes.data,
                                                  m2.ctypes.data))

    def index_remove(self, uuid: str):
        self._chk(lib().tfp_group_index_remove(self._h, uuid.encode()))

    def index_clear(self):
        self._chk(lib().tfp_group_index_clear(self._h))

    def index_rows(self, uuid: str):
        n = C.c_int64()
        rc = lib().tfp_group_index_rows(self._h, uuid.encode(), None, None, 0, C.byref(n))
        if rc not in (0, -5):
            self._chk(rc)
        m1 = np.zeros(max(n.value, 1), np.int32)
        m2 = np.zeros(max(n.value, 1), np.int32)
        self._chk(lib().tfp_group_index_rows(self._h, uuid.encode(), m1.ctypes.data, m2.ctypes.data, n.value,
                                             C.byref(n)))
        return m1[:n.value], m2[:n.value]

    def index_stats(self):
        r, c = C.c_int64(), C.c_int32()
        self._chk(lib().tfp_group_index_stats(self._h, C.byref(r), C.byref(c)))
        return r.value, c.value

    def index_commit(self):
        self._chk(lib().tfp_group_index_commit(self._h))

    def search_batch(self, frames: np.ndarray, qoffsets, p: SearchParams):
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq = len(qoffsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_group_search_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p), res))
        return Engine._results(res, nq)

    def search_pcm_batch(self, pcm, offsets, p: SearchParams, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_group_search_pcm_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                   C.byref(p), res))
        return Engine._results(res, nq)

    def search_g711_batch(self, codes, offsets, law: int, p: SearchParams, sample_rate: int = 8000):
        codes = np.ascontiguousarray(codes, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_group_search_g711_batch(self._h, codes.ctypes.data, offsets.ctypes.data, nq, int(law),
                                                    sample_rate, C.byref(p), res))
        return Engine._results(res, nq)

    def search_f32_batch(self, x, offsets, p: SearchParams, sample_rate: int = 8000):
        x = np.ascontiguousarray(x, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq = len(offsets) - 1
        res = (Result * max(1, nq))()
        self._chk(lib().tfp_group_search_f32_batch(self._h, x.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                   C.byref(p), res))
        return Engine._results(res, nq)

    def search_ranked_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, k: int):
        """Engine.search_ranked_batch over every shard's clips (clip_id = the shard holding the clip)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_group_search_ranked_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p),
                                                      k, out, counts))
        return Engine._candidates(out, counts, nq, k)

    def search_aligned_batch(self, frames: np.ndarray, qoffsets, p: SearchParams, k: int):
        """Engine.search_aligned_batch over every shard's clips, each row aligned on the shard holding its clip."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        qoffsets = np.ascontiguousarray(qoffsets, np.int64)
        nq, k = len(qoffsets) - 1, int(k)
        n = max(1, nq * max(k, 1))
        out, align, counts = (Candidate * n)(), (Alignment * n)(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_group_search_aligned_batch(self._h, frames.ctypes.data, qoffsets.ctypes.data, nq, C.byref(p),
                                                       k, out, align, counts))
        return Engine._aligned(out, align, counts, nq, k)

    def search_ranked_pcm_batch(self, pcm, offsets, p: SearchParams, k: int, sample_rate: int = 8000):
        pcm = np.ascontiguousarray(pcm, np.int16)
        offsets = np.ascontiguousarray(offsets, np.int64)
        nq, k = len(offsets) - 1, int(k)
        out, counts = (Candidate * max(1, nq * max(k, 1)))(), (C.c_int32 * max(1, nq))()
        self._chk(lib().tfp_group_search_ranked_pcm_batch(self._h, pcm.ctypes.data, offsets.ctypes.data, nq, sample_rate,
                                                          C.byref(p), k, out, counts))
        return Engine._candidates(out, counts, nq, k)

    def scope_stats(self) -> dict:
        """Engine.scope_stats summed over the shards' engines."""
        tot = {"vote_batches": 0, "general_batches": 0, "table_builds": 0}
        for s in range(self.size()):
            v, g, t = C.c_int64(), C.c_int64(), C.c_int64()
            check(lib().tfp_scope_stats(lib().tfp_group_engine(self._h, s), C.byref(v), C.byref(g), C.byref(t)))
            for key, x in zip(tot, (v, g, t)):
                tot[key] += x.value
        return tot

    def neighbour_stats(self) -> dict:
        """Engine.neighbour_stats summed over the shards' engines."""
        tot = {"vote_batches": 0, "general_batches": 0, "pairs_aligned": 0, "frames_read": 0}
        for s in range(self.size()):
            x = [C.c_int64() for _ in tot]
            check(lib().tfp_neighbour_stats(lib().tfp_group_engine(self._h, s), *[C.byref(v) for v in x]))
            for key, v in zip(tot, x):
                tot[key] += v.value
        return tot


class GroupStream:
    """tfp_group_stream: live channels matched against every shard of a Group."""

    def __init__(self, g: Group, nchannels: int, window_samples: int, sample_rate: int = 8000):
        self._g = g
        self._h = C.c_void_p()
        g._chk(lib().tfp_group_stream_create(g.handle, int(nchannels), int(sample_rate), int(window_samples),
                                             C.byref(self._h)))
        self.nchannels = nchannels
        self._res = (Result * nchannels)()
        g._streams.add(self)

    def reset(self, channel: int = -1):
        self._g._chk(lib().tfp_group_stream_reset(self._h, int(channel)))

    def push(self, pcm: np.ndarray, p: SearchParams = None):
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.shape[0] == self.nchannels
        self._g._chk(lib().tfp_group_stream_push(self._h, pcm.ctypes.data, pcm.shape[1],
                                                 C.byref(p) if p is not None else None,
                                                 self._res if p is not None else None))
        if p is None:
            return None
        return [None if not r.found else {"audio_uuid": r.uuid.decode(), "match_count": r.match_count,
                                          "frame_count": r.frame_count} for r in self._res]

    def push_g711(self, codes: np.ndarray, law: int, p: SearchParams = None):
        codes = np.ascontiguousarray(codes, np.uint8)
        assert codes.shape[0] == self.nchannels
        self._g._chk(lib().tfp_group_stream_push_g711(self._h, codes.ctypes.data, codes.shape[1], int(law),
                                                      C.byref(p) if p is not None else None,
                                                      self._res if p is not None else None))
        if p is None:
            return None
        return [None if not r.found else {"audio_uuid": r.uuid.decode(), "match_count": r.match_count,
                                          "frame_count": r.frame_count} for r in self._res]

    def close(self):
        if self._h and self._g._h:
            lib().tfp_group_stream_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupLive(_LiveCalls):
    """tfp_group_live: live calls matched against every shard of a Group (every shard keeps every channel)."""
    _PFX = "tfp_group_live"

    def __init__(self, g: Group, nchannels: int, max_samples: int, sample_rate: int = 8000, rate_in: int = None):
        """rate_in: the rate the ticks arrive at (tfp_group_live_create_rate); None: a plain object."""
        self._open(g, nchannels, max_samples, sample_rate, rate_in)

    def rate_stats(self) -> list:
        """tfp_group_live_rate_stats: each shard's tfp_live_rate_stats, in shard order."""
        return [self._rate_stats(shard) for shard in range(len(self._owner.devices))]

    def stats(self) -> list:
        """tfp_group_live_stats: each shard's tfp_live_stats, in shard order."""
        res = []
        for shard in range(len(self._owner.devices)):
            v = [C.c_int64() for _ in range(5)]
            self._owner._chk(lib().tfp_group_live_stats(self._h, shard, *[C.byref(x) for x in v]))
            res.append(dict(zip(("incremental_pushes", "general_pushes", "rebuilds", "frames_fingerprinted",
                                 "frames_added"), (x.value for x in v))))
        return res

    def window_stats(self) -> list:
        """tfp_group_live_window_stats: each shard's tfp_live_window_stats, in shard order."""
        return [self._window_stats(shard) for shard in range(len(self._owner.devices))]

    def window_aligned_stats(self) -> list:
        """tfp_group_live_window_aligned_stats: each shard's tfp_live_window_aligned_stats, in shard order."""
        return [self._window_aligned_stats(shard) for shard in range(len(self._owner.devices))]

    def occurrence_stats(self) -> list:
        """tfp_group_live_occurrence_stats: each shard's tfp_live_occurrence_stats, in shard order."""
        return [self._occurrence_stats(shard) for shard in range(len(self._owner.devices))]
