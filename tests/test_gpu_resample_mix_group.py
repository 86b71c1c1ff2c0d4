"""The multichannel rate forms on a device group (tfp_group_fingerprint_mix_rate_batch,
tfp_group_search_mix_rate_batch, tfp_group_search_scoped_mix_rate_batch) equal the single-engine forms on a
ragged batch, on devices 0,0,0; the clips are cut across the shards by their frames at rate_out."""
import numpy as np
import pytest

from resample_mix_util import mix_noise, pack
from resample_util import TILE, bits_equal, edge_lengths, ragged_order

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
    devices = [0, 0, 0]
    g, e = Group(devices), tfp_lib.Engine(0)
    try:
        rin, rout = 44100, 8000
        order = ragged_order(edge_lengths(tfp_lib.resample_taps(rin, rout), TILE))
        for ch in (2, 3):
            clips = [mix_noise(n, ch, 7 + n) for n in order]
            pcm, off = pack(clips, ch)
            m0 = g.resample_mix_stats()
            bits_equal(g.fingerprint_mix_rate_batch(pcm, off, ch, rin, rout), e.fingerprint_mix_rate_batch(pcm, off, ch, rin, rout))
            m1 = g.resample_mix_stats()
            # each shard converts the clips it fingerprints: consecutive runs cut where the frames at rate_out
            # pass s / 3 of the total (tfp_group_fingerprint_rate_batch's cut)
            nf = [tfp_lib.frame_count(max(tfp_lib.resample_count(n, rin, rout), 0)) for n in order]
            foff = np.concatenate([[0], np.cumsum(nf)])
            cut = [0] + [int(np.searchsorted(foff, foff[-1] * s // 3, "left")) for s in (1, 2)] + [len(order)]
            for s in range(3):
                a, b = cut[s], cut[s + 1]
                d = {k: m1[s][k] - m0[s][k] for k in m0[s]}
                assert d["frames_in"] == sum(order[a:b]), (s, d, cut)
                assert d["launches"] == d["staged_launches"] == (1 if sum(order[a:b]) else 0)
            assert all(m1[s]["frames_in"] > m0[s]["frames_in"] for s in range(3))  # every shard took a share
            bits_equal(g.fingerprint_mix_rate_batch(pcm, off, ch, 8000, 8000), e.fingerprint_mix_rate_batch(pcm, off, ch, 8000, 8000))
        nclips, n = 24, 8000 * 3
        src = tfp_lib.synth_pcm(SEED_DB, range(nclips), n)
        fr = e.fingerprint_batch(src.reshape(-1), np.arange(nclips + 1, dtype=np.int64) * n)
        nf = tfp_lib.frame_count(n)
        uuids = [_uuid(c) for c in range(nclips)]
        for c in range(nclips):
            f = fr[c * nf:(c + 1) * nf]
            e.index_add(uuids[c], f["m1"], f["m2"])
            g.index_add(uuids[c], f["m1"], f["m2"])
        for h in (e, g):
            h.index_set_scope(uuids, [c % 3 for c in range(nclips)])
        qs = []
        for i in range(9):
            up = tfp_lib.resample_pcm(src[(5 * i) % nclips, 256 * (2 + i):256 * (2 + i) + 7000 + 301 * i], 8000, 16000)
            qs.append(np.stack([up, up // 2, -(up // 3)], 1).astype(np.int16))
        qs.append(np.zeros((0, 3), np.int16))
        qpcm, qoff = pack(qs, 3)
        scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            rg, fcg = g.search_mix_rate_batch(qpcm, qoff, 3, 16000, 8000, p)
            re_, fce = e.search_mix_rate_batch(qpcm, qoff, 3, 16000, 8000, p)
            assert [_key(r) for r in rg] == [_key(r) for r in re_] and fcg == fce
            sg, sfg = g.search_scoped_mix_rate_batch(qpcm, qoff, 3, 16000, 8000, p, scopes, 3)
            se, sfe = e.search_scoped_mix_rate_batch(qpcm, qoff, 3, 16000, 8000, p, scopes, 3)
            assert _rows(sg) == _rows(se) and sfg == sfe
        with pytest.raises(tfp_lib.TfpError, match="unsupported channel count"):
            g.search_mix_rate_batch(qpcm, qoff, 33, 16000, 8000, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="unsupported rate ratio"):
            g.search_mix_rate_batch(qpcm, qoff, 3, 7999, 44100, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="bad sample rate"):
            g.fingerprint_mix_rate_batch(qpcm, qoff, 3, 0, 8000)
    finally:
        g.close()
        e.close()
