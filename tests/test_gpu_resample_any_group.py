"""Mixed batches on a device group (tfp_group_fingerprint_any_batch, tfp_group_search_any_batch,
tfp_group_search_scoped_any_batch) equal the single-engine forms, on devices 0,0 and 0,0,0: a fingerprint batch is
cut across the shards by its frames at rate_out, with clips of different classes on both sides of every cut and one
conversion launch per shard that has output; every shard converts a search batch."""
import numpy as np
import pytest

from resample_any_util import ALAW, Q31, S16, ULAW, key as _key, render, samples, uuid as _uuid
from resample_util import TILE, bits_equal, class_clip

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.001), (1, 0.45), (2, 0.45)]


def _rows(rows):
    return [[(r["audio_uuid"], r["match_count"]) for r in q] for q in rows]


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["0,0", "0,0,0"])
def test_group_equals_one_engine(tfp_lib, devices):
    from tiresias_amd import Group
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    g, e = Group(devices), tfp_lib.Engine(0)
    try:
        # twelve clips, the classes in rotation, so every run of three or more holds several classes
        classes = [(S16, 1, 16000), (Q31, 2, 44100), (ULAW, 1, 16000), (S16, 2, 44100), (ALAW, 1, 8000), (Q31, 1, 48000)]
        lens = [2 * TILE + 5, 700, TILE, 0, 3001, TILE + 1, 2600, 1, 2 * TILE, 1500, 900, 2222]  # outputs at 8000, about
        items = [(samples(k, n * r // 8000, ch, 3 + i), r, k)
                 for i, (n, (k, ch, r)) in enumerate(zip(lens, classes * 2))]
        data, clips = tfp_lib.pack_audio_clips(items)
        a0 = g.resample_any_stats()
        bits_equal(g.fingerprint_any_batch(data, clips, 8000), e.fingerprint_any_batch(data, clips, 8000))
        a1 = g.resample_any_stats()
        nout = tfp_lib.audio_clips_check(clips, len(data), 8000)
        foff = np.concatenate([[0], np.cumsum([tfp_lib.frame_count(int(n)) for n in nout])])
        ns = len(devices)
        cut = [0] + [int(np.searchsorted(foff, foff[-1] * s // ns, "left")) for s in range(1, ns)] + [len(items)]
        for s in range(ns):
            a, b = cut[s], cut[s + 1]
            d = {k: a1[s][k] - a0[s][k] for k in a0[s]}
            assert b - a >= 3 and len({int(k) for k in clips["kind"][a:b]}) >= 2, cut  # several classes per shard
            assert d["launches"] == 1 and d["clips"] == b - a, (s, d, cut)
            assert d["frames_in"] == int(clips["nframes"][a:b].sum()) and d["samples_out"] == int(nout[a:b].sum())
        n = 8000 * 2
        src = [class_clip(k, n) for k in (0, 1, 2)] + list(tfp_lib.synth_pcm(0x7153A1, range(9), n))
        uuids = [_uuid(c) for c in range(len(src))]
        for u, c in zip(uuids, src):
            f = e.fingerprint_batch(c, [0, n], 8000)
            e.index_add(u, f["m1"], f["m2"])
            g.index_add(u, f["m1"], f["m2"])
        for h in (e, g):
            h.index_set_scope(uuids, [c % 3 for c in range(len(src))])
        qs = [render(tfp_lib, c[256 * (2 + i):256 * (2 + i) + 7000 + 301 * i], i % 4, i) for i, c in enumerate(src)]
        qs.append((samples(ULAW, 0, 1, 1), 16000, ULAW))
        qd, qc = tfp_lib.pack_audio_clips(qs)
        scopes = [(-1 if i % 4 == 3 else i % 3) for i in range(len(qs))]
        for coefs, tol in PARAMS:
            p = tfp_lib.params(coefs, tol)
            s0 = g.resample_any_stats()
            rg, fcg = g.search_any_batch(qd, qc, 8000, p)
            assert [x["launches"] - y["launches"] for x, y in zip(g.resample_any_stats(), s0)] == [1] * ns
            re_, fce = e.search_any_batch(qd, qc, 8000, p)
            assert [_key(r) for r in rg] == [_key(r) for r in re_] and fcg == fce
            sg, sfg = g.search_scoped_any_batch(qd, qc, 8000, p, scopes, 3)
            se, sfe = e.search_scoped_any_batch(qd, qc, 8000, p, scopes, 3)
            assert _rows(sg) == _rows(se) and sfg == sfe
            assert sfg == [tfp_lib.frame_count(int(x)) for x in tfp_lib.audio_clips_check(qc, len(qd), 8000)]
        bad = qc.copy()
        bad["channels"][2] = 33
        with pytest.raises(tfp_lib.TfpError, match="clip 2: unsupported channel count 33"):
            g.search_any_batch(qd, bad, 8000, tfp_lib.params(1, 0.45))
        with pytest.raises(tfp_lib.TfpError, match="clip 0: unsupported rate ratio 16000 -> 44099"):
            g.fingerprint_any_batch(qd, qc, 44099)
        with pytest.raises(tfp_lib.TfpError, match="bad sample rate 0"):
            g.search_scoped_any_batch(qd, qc, 0, tfp_lib.params(1, 0.45), scopes, 3)
    finally:
        g.close()
        e.close()
