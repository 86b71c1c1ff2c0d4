"""The wide (int32 Q31) rate forms on a device group (tfp_group_fingerprint_wide_rate_batch,
tfp_group_search_wide_rate_batch, tfp_group_search_scoped_wide_rate_batch) equal the single-engine forms on a
ragged batch, on devices 0,0; the clips are cut across the shards by their frames at rate_out."""
import numpy as np
import pytest

from resample_util import TILE, bits_equal, class_clip, in_len_for
from resample_wide_util import pack, wide_noise

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]
SEED_DB = 0x7153A1


def _uuid(c):
    return "%08x-7a7e-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def _rows(rows):
    return [[(r["audio_uuid"], r["match_count"]) for r in q] for q in rows]


def test_group_equals_one_engine(tfp_lib):
    from tiresias_amd import Group
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    g, e = Group([0, 0]), tfp_lib.Engine(0)
    try:
        rin, rout = 44100, 8000
        t = tfp_lib.resample_taps(rin, rout)
        order = [0, 1, t["ntaps"] - 1, in_len_for(TILE, t["L"], t["M"]), 2 * t["ntaps"] + 1, in_len_for(TILE + 1, t["L"], t["M"]), 700, 0,
                 in_len_for(2 * TILE + 1, t["L"], t["M"])]
        for ch in (1, 2, 3):
            clips = [wide_noise(n, ch, 7 + n) for n in order]
            q, off = pack(clips, ch)
            w0 = g.resample_wide_stats()
            bits_equal(g.fingerprint_wide_rate_batch(q, off, ch, rin, rout), e.fingerprint_wide_rate_batch(q, off, ch, rin, rout))
            w1 = g.resample_wide_stats()
            # each shard converts the clips it fingerprints: consecutive runs cut where the frames at rate_out
            # pass half of the total (tfp_group_fingerprint_rate_batch's cut)
            nf = [tfp_lib.frame_count(max(tfp_lib.resample_count(n, rin, rout), 0)) for n in order]
            foff = np.concatenate([[0], np.cumsum(nf)])
            cut = [0, int(np.searchsorted(foff, foff[-1] // 2, "left")), len(order)]
            for s in range(2):
                a, b = cut[s], cut[s + 1]
                d = {k: w1[s][k] - w0[s][k] for k in w0[s]}
                assert d["frames_in"] == sum(order[a:b]), (s, d, cut)
                assert d["launches"] == d["staged_launches"] == (1 if sum(order[a:b]) else 0)
            assert all(w1[s]["frames_in"] > w0[s]["frames_in"] for s in range(2))  # every shard took a share
            bits_equal(g.fingerprint_wide_rate_batch(q, off, ch, 8000, 8000), e.fingerprint_wide_rate_batch(q, off, ch, 8000, 8000))
        n = 8000 * 3
        src = [class_clip(k, n) for k in (0, 1, 2)] + list(tfp_lib.synth_pcm(SEED_DB, range(5), n))
        uuids = [_uuid(c) for c in range(len(src))]
        for u, c in zip(uuids, src):
            f = e.fingerprint_batch(c, [0, n], 8000)
            e.index_add(u, f["m1"], f["m2"])
            g.index_add(u, f["m1"], f["m2"])
        for h in (e, g):
            h.index_set_scope(uuids, [c % 3 for c in range(len(src))])
        qs = []
        for i, c in enumerate(src):
            up = tfp_lib.resample_pcm(c[256 * (2 + i):256 * (2 + i) + 7000 + 301 * i], 8000, 16000).astype(np.int32) << 16
            qs.append(np.stack([up, up // 2, -(up // 3)], 1).astype(np.int32) + 12345)
        qs.append(np.zeros((0, 3), np.int32))
        q, qoff = pack(qs, 3)
        scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            rg, fcg = g.search_wide_rate_batch(q, qoff, 3, 16000, 8000, p)
            re_, fce = e.search_wide_rate_batch(q, qoff, 3, 16000, 8000, p)
            assert [_key(r) for r in rg] == [_key(r) for r in re_] and fcg == fce
            sg, sfg = g.search_scoped_wide_rate_batch(q, qoff, 3, 16000, 8000, p, scopes, 3)
            se, sfe = e.search_scoped_wide_rate_batch(q, qoff, 3, 16000, 8000, p, scopes, 3)
            assert _rows(sg) == _rows(se) and sfg == sfe
            assert sfg == [tfp_lib.frame_count(max(tfp_lib.resample_count(len(x), 16000, 8000), 0)) for x in qs]
        with pytest.raises(tfp_lib.TfpError, match="unsupported channel count"):
            g.search_wide_rate_batch(q, qoff, 33, 16000, 8000, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="unsupported rate ratio"):
            g.search_wide_rate_batch(q, qoff, 3, 7999, 44100, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="bad sample rate"):
            g.fingerprint_wide_rate_batch(q, qoff, 3, 0, 8000)
    finally:
        g.close()
        e.close()
