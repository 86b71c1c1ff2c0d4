"""The rate forms on a device group (tfp_group_fingerprint_rate_batch, tfp_group_search_rate_batch,
tfp_group_search_scoped_rate_batch) equal the single-engine forms, on devices 0,0 and 0,0,0."""
import numpy as np
import pytest

from resample_util import bits_equal, noise

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]
SEED_DB = 0x7153A1


def _uuid(c):
    return "%08x-7a7e-4000-8000-%012x" % (c * 2654435761 % 2**32, c)


def _key(r):
    return None if r is None else (r["audio_uuid"], r["match_count"], r["frame_count"])


def _rows(rows):
    return [[(r["audio_uuid"], r["match_count"]) for r in q] for q in rows]


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["0,0", "0,0,0"])
def test_group_equals_one_engine(tfp_lib, devices):
    from tiresias_amd import Group
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    g, e = Group(devices), tfp_lib.Engine(0)
    try:
        rin, rout = 44100, 8000
        lens = [0, 1, 5000, 265, 12000, 266, 3, 20000, 7001]
        pcm = noise(sum(lens), 4)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        r0 = g.resample_stats()
        bits_equal(g.fingerprint_rate_batch(pcm, off, rin, rout), e.fingerprint_rate_batch(pcm, off, rin, rout))
        r1 = g.resample_stats()
        assert r1["samples_in"] - r0["samples_in"] == len(pcm)  # each shard converts what it fingerprints
        assert 1 <= r1["launches"] - r0["launches"] <= len(devices)
        bits_equal(g.fingerprint_rate_batch(pcm, off, 8000, 8000), e.fingerprint_batch(pcm, off, 8000))
        nclips, n = 24, 8000 * 3
        clips = tfp_lib.synth_pcm(SEED_DB, range(nclips), n)
        fr = e.fingerprint_batch(clips.reshape(-1), np.arange(nclips + 1, dtype=np.int64) * n)
        nf = tfp_lib.frame_count(n)
        uuids = [_uuid(c) for c in range(nclips)]
        for c in range(nclips):
            f = fr[c * nf:(c + 1) * nf]
            e.index_add(uuids[c], f["m1"], f["m2"])
            g.index_add(uuids[c], f["m1"], f["m2"])
        for h in (e, g):
            h.index_set_scope(uuids, [c % 3 for c in range(nclips)])
        qs = [tfp_lib.resample_pcm(clips[(5 * i) % nclips, 256 * (2 + i):256 * (2 + i) + 7000 + 301 * i], 8000, 16000)
              for i in range(9)] + [np.zeros(0, np.int16)]
        qpcm = np.concatenate(qs)
        qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
        scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            rg, fcg = g.search_rate_batch(qpcm, qoff, 16000, 8000, p)
            re_, fce = e.search_rate_batch(qpcm, qoff, 16000, 8000, p)
            assert [_key(r) for r in rg] == [_key(r) for r in re_] and fcg == fce
            sg, sfg = g.search_scoped_rate_batch(qpcm, qoff, 16000, 8000, p, scopes, 3)
            se, sfe = e.search_scoped_rate_batch(qpcm, qoff, 16000, 8000, p, scopes, 3)
            assert _rows(sg) == _rows(se) and sfg == sfe
        with pytest.raises(tfp_lib.TfpError, match="unsupported rate ratio"):
            g.search_rate_batch(qpcm, qoff, 7999, 44100, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="bad sample rate"):
            g.fingerprint_rate_batch(pcm, off, 0, 8000)
    finally:
        g.close()
        e.close()
