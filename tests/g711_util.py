"""G.711 for the tests: the two 16-bit expansions in numpy (the formulas libsndfile, Asterisk and
Python's audioop share), an encoder good enough to make test audio, and WAV bytes around codes."""
import struct

import numpy as np

ULAW, ALAW = 0, 1

# code -> value anchors of the issue (mu-law range +-32124, A-law +-32256)
ANCHORS = {
    ULAW: {0x00: -32124, 0x80: 32124, 0x7E: -8, 0xFE: 8, 0x7F: 0, 0xFF: 0},
    ALAW: {0x55: -8, 0xD5: 8, 0x2A: -32256, 0xAA: 32256, 0x00: -5504, 0x80: 5504},
}


def ulaw_expand(codes) -> np.ndarray:
    c = (~np.asarray(codes, np.uint8)).astype(np.int32) & 0xFF
    t = (((c & 0x0F) << 3) + 0x84) << ((c & 0x70) >> 4)
    return np.where(c & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw_expand(codes) -> np.ndarray:
    c = (np.asarray(codes, np.uint8).astype(np.int32) ^ 0x55) & 0xFF
    t = (c & 0x0F) << 4
    seg = (c & 0x70) >> 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(c & 0x80, t, -t).astype(np.int16)


def expand(codes, law: int) -> np.ndarray:
    return alaw_expand(codes) if law == ALAW else ulaw_expand(codes)


def encode(pcm, law: int) -> np.ndarray:
    """The code whose expansion is nearest to each int16 sample (ties to the lower code). Any
    encoder would do for the tests: what they compare is always the expansion of these codes."""
    table = expand(np.arange(256, dtype=np.uint8), law).astype(np.int32)
    order = np.argsort(table, kind="stable")
    vals = table[order]
    x = np.asarray(pcm, np.int32)
    j = np.clip(np.searchsorted(vals, x), 1, 255)
    j = np.where(np.abs(vals[j - 1] - x) <= np.abs(vals[j] - x), j - 1, j)
    return order[j].astype(np.uint8)


def chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt(tag: int, channels: int = 1, rate: int = 8000, bits: int = 8, align=None) -> bytes:
    align = channels * max(bits // 8, 1) if align is None else align
    return chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits))


def fmt_ext(sub_tag: int, channels: int = 1, rate: int = 8000, bits: int = 8) -> bytes:
    align = channels * max(bits // 8, 1)
    guid = struct.pack("<H", sub_tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    return chunk(b"fmt ", struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits, 4) + guid)


def riff(*chunks: bytes) -> bytes:
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def wav_tag(law: int) -> int:
    return 6 if law == ALAW else 7


def g711_wav(codes, law: int, rate: int = 8000, extensible: bool = False) -> bytes:
    data = chunk(b"data", np.asarray(codes, np.uint8).tobytes())
    head = fmt_ext(wav_tag(law), rate=rate) if extensible else fmt(wav_tag(law), rate=rate)
    return riff(head, data)
