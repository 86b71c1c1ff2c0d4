"""Live calls at scale (tfp_live_*, csrc/tfp_live.hip): the 16-bit count rows, added in pairs as 32-bit
words, across 255 -> 256, 32767 -> 32768 and up to the 65535 final frames a channel may hold; and a
catch-up push large enough for the 16-frame throughput fingerprint launch, with a lead-in frame to
drop, history rows that start on odd samples and ends off the hop. Every push equals
tfp_search_scoped_pcm_batch on the samples the channel has taken so far (live_util.check_push)."""
import numpy as np
import pytest

import live_util as L

pytestmark = pytest.mark.gpu

TFP_E_CAPACITY = -5
HOP = 256
CAP = 65535 * HOP  # kLiveMaxSamples


def _keys(frames):
    return [int(v) if np.isfinite(v) else 0 for v in frames["q1"]]  # (int) truncation, fp_handler.c:290


def _tail_key(engine, call, s):
    """The key of the provisional frame of call[:s]: it reads [256 (f - 1), s) and zeros after."""
    f = s // HOP
    return _keys(engine.fingerprint(call[max(0, HOP * (f - 1)):s]))[-1]


def test_count_rows_up_to_65535_frames(engine, tfp_lib):
    """Two channels up to 65535 final frames. 32 clips, all returned (k = 32): in columns 0 ... 27 the even
    column has a row in every key the calls' frames take (its count is every frame) and its odd neighbour
    a row in one rare key only; columns 28 ... 31 have it the other way round. The pair shares a 32-bit
    word of the count row, so a carry out of a half-word, or an add into the wrong half, shows in a
    returned row. The pushes step channel 0's final frames over 255 -> 256 -> 257 and 32767 -> 32768 ->
    32769, then to 65534 with a tail (score = count + the tail's bit = 65535), then to 65535."""
    seg = tfp_lib.synth_pcm(0x5CA1E, [0], 9001)[0]  # an odd period: every frame phase occurs
    call = np.tile(seg, CAP // len(seg) + 2)
    calls = [call[:CAP], call[77:77 + CAP]]
    # cumulative samples per push: (channel 0, channel 1); channel 1 lags and crosses the same steps later
    steps = [(255 * HOP + 17, 100), (256 * HOP + 5, 255 * HOP), (257 * HOP, 256 * HOP + 1),
             (32767 * HOP + 100, 257 * HOP + 255), (32768 * HOP + 3, 20000 * HOP + 7),
             (32769 * HOP, 32767 * HOP + 255), (65534 * HOP + 100, 32768 * HOP), (CAP, 40000 * HOP + 13)]
    # the index: a row per key the calls take (every final frame, and channel 0's tails)
    count = {}
    for c in (0, 1):
        for k in _keys(engine.fingerprint(calls[c][:steps[-1][c]])):
            count[k] = count.get(k, 0) + 1
    for s0, _ in steps:
        if s0 % HOP:
            count.setdefault(_tail_key(engine, calls[0], s0), 0)
    keys = sorted(count)
    rare = min((k for k in keys if count[k]), key=lambda k: (count[k], k))
    assert len(keys) > 1 and 0 < count[rare] < 65535
    n = 32
    uuids = ["00000000-6666-4000-8000-%012d" % c for c in range(n)]  # column = c
    full = [c for c in range(n) if (c % 2 == 0) == (c < 28)]
    engine.index_clear()
    for c in range(n):
        ks = keys if c in full else [rare]
        engine.index_add(uuids[c], np.array([k * 1_000_000 + 500 for k in ks], np.int32), np.zeros(len(ks), np.int32))
    engine.index_set_scope(uuids, [0] * n)
    scopes = [0, -1]
    p = tfp_lib.params(1, 0.001)
    lv = tfp_lib.Live(engine, 2, CAP)
    hist = [np.zeros(0, np.int16) for _ in range(2)]
    at = [0, 0]
    try:
        for s in steps:
            nn = [s[c] - at[c] for c in range(2)]
            blk = np.zeros((2, max(nn)), np.int16)
            for c in range(2):
                blk[c, :nn[c]] = calls[c][at[c]:s[c]]
                at[c] = s[c]
            rows = L.check_push(tfp_lib, engine, lv, hist, blk, p, scopes, n, nsamples=nn, where=s)
            # the edge itself, on counts the prefix search gave as well: every frame counts for the full columns
            assert [r["audio_uuid"] for r in rows[0][:16]] == [uuids[c] for c in reversed(full)], s
            assert all(r["match_count"] == -(-s[0] // HOP) for r in rows[0][:16]), s
            assert all(r["match_count"] < s[0] // HOP for r in rows[0][16:]), s
            if s[1] >= HOP:
                assert [r["match_count"] >= s[1] // HOP for r in rows[1]] == [True] * 16 + [False] * (len(rows[1]) - 16), s
        assert len(rows[0]) == n and len(rows[1]) == n  # the rare key's columns too, with small counts
        assert rows[0][0]["match_count"] == 65535 and 0 < rows[0][16]["match_count"] < 65535 and lv.samples(0) == CAP
        st = lv.stats()
        assert st["general_pushes"] == 0 and st["rebuilds"] == 1 and st["incremental_pushes"] == len(steps)
        assert st["frames_added"] == sum(a // HOP for a in at)
        v = lv.verdict([CAP, at[1]], p, scopes)
        assert v[0]["complete"] and v[0]["decided"]
        assert (v[0]["leader"]["audio_uuid"], v[0]["leader"]["match_count"]) == (uuids[31], 65535)
        assert (v[0]["rival"]["audio_uuid"], v[0]["rival"]["match_count"]) == (uuids[29], 65535)
        # one more sample: all or nothing
        with pytest.raises(tfp_lib.TfpError) as ei:
            lv.push(np.zeros((2, 1), np.int16), p, scopes, n, nsamples=[1, 0])
        assert ei.value.code == TFP_E_CAPACITY
        assert [lv.samples(c) for c in range(2)] == at
        # another tolerance: the table is rebuilt from the 65535 kept frames in one add
        p2 = tfp_lib.params(1, 0.002)
        rows = L.check_push(tfp_lib, engine, lv, hist, np.zeros((2, 1), np.int16), p2, scopes, n, nsamples=[0, 0],
                            where="rebuild")
        assert rows[0][0]["match_count"] == 65535
        st = lv.stats()
        assert st["general_pushes"] == 0 and st["rebuilds"] == 2
        assert st["frames_added"] == 2 * sum(a // HOP for a in at)
    finally:
        lv.close()
        engine.index_clear()


def _codes(tfp_lib, pcm, law):
    table = tfp_lib.decode_g711(np.arange(256, dtype=np.uint8), law).astype(np.int32)
    order = np.argsort(table, kind="stable")
    return order[np.clip(np.searchsorted(table[order], pcm.astype(np.int32)), 0, 255)].astype(np.uint8)


@pytest.mark.parametrize("law", [None, "ulaw"])
def test_catch_up_push_takes_the_throughput_launch(engine, tfp_lib, law):
    """Ingest-only pushes of sizes that differ per channel and are no multiples of the hop, then one
    searching push of more than 4096 frames in all: live_step's rule (more than 256 tiles of 16 frames)
    takes the throughput launch, with a lead-in frame on every channel, clips that begin inside history
    rows of an odd length, and ends off the hop. Rows equal the prefix search; a coefs = 2 push of no
    samples compares the kept frame values."""
    L.build_db(tfp_lib, engine)
    big = 520 * HOP + 77
    cap = 140001  # odd: channel c's history row starts on sample c * 140001
    ingest = [[300 + 37 * c for c in range(8)], [515 + 11 * c for c in range(8)], [1 + c for c in range(8)]]
    final = [big + 3 * c for c in range(8)]
    total = [sum(x[c] for x in ingest) + final[c] for c in range(8)]
    assert max(total) <= cap and all(sum(x[c] for x in ingest) >= HOP for c in range(8))  # a lead-in frame everywhere
    assert sum((-(-(total[c] - HOP * (sum(x[c] for x in ingest) // HOP - 1)) // HOP) + 15) // 16 for c in range(8)) > 256
    # windows of enrolled clips (beyond their enrolled length too), noise and silence
    src = tfp_lib.synth_pcm(L.SEED, [L.TWIN[0], 7, 12, 20, 33, 3], cap, offsets=[1024, 333, 1, 777, 2049, 1535])
    src = np.concatenate([src, tfp_lib.synth_pcm(0xBEEF, [0], cap), np.zeros((1, cap), np.int16)])
    if law:
        codes = _codes(tfp_lib, src, tfp_lib.ULAW)
        src = tfp_lib.decode_g711(codes.reshape(-1), tfp_lib.ULAW).reshape(8, cap)

    def push(lv, at, nn, *args):
        blk = np.zeros((8, max(max(nn), 1)), np.int16)
        for c in range(8):
            blk[c, :nn[c]] = src[c, at[c]:at[c] + nn[c]]
            blk[c, nn[c]:] = 12345  # past nsamples[c]: never read
        if law:
            return lv.push_g711(_codes(tfp_lib, blk, tfp_lib.ULAW), tfp_lib.ULAW, *args, nsamples=nn)
        return lv.push(blk, *args, nsamples=nn)

    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, cap)
    at = [0] * 8
    try:
        for nn in ingest:
            assert push(lv, at, nn, None) is None
            at = [a + x for a, x in zip(at, nn)]
        s0 = engine.fingerprint_stats()
        rows, fc = push(lv, at, final, p, L.SCOPES8, 32)
        s1 = engine.fingerprint_stats()
        assert {k: s1[k] - s0[k] for k in s1} == {"small8k": 0, "throughput8k": 1, "generic_i16": 0, "generic_f32": 0}
        at = [a + x for a, x in zip(at, final)]
        assert at == total
        hist = [src[c, :total[c]] for c in range(8)]
        exp = L.prefix_rows(engine, hist, p, L.SCOPES8, 32)
        assert fc == [tfp_lib.frame_count(t) for t in total]
        for c in range(8):
            assert rows[c] == exp[c], c
        assert rows[0] and rows[0][0]["match_count"] > 0  # the calls do match clips
        st = lv.stats()
        assert st["incremental_pushes"] == 1 and st["general_pushes"] == 0 and st["rebuilds"] == 1
        assert st["frames_added"] == sum(t // HOP for t in total)
        # the kept frame values themselves: coefs = 2 boxes the second value of each
        hist = [h.copy() for h in hist]
        L.check_push(tfp_lib, engine, lv, hist, np.zeros((8, 1), np.int16), tfp_lib.params(2, 0.1), L.SCOPES8, 3,
                     nsamples=[0] * 8, where="values")
        assert lv.stats()["general_pushes"] == 1
    finally:
        lv.close()
        engine.index_clear()
