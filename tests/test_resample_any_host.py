"""tfp_resample_any_pcm, the host definition of a mixed batch's clip: the existing host map of the clip's class
(tfp_resample_pcm, tfp_resample_mix_pcm, tfp_resample_wide_pcm, tfp_g711_decode then tfp_resample_pcm), bit for bit,
for each kind at every pair the mixed forms are built for, at equal rates, and at the lengths where the filter's
ends matter. No GPU."""
import numpy as np
import pytest

from resample_any_util import ALAW, Q31, S16, ULAW, class_map, samples

PAIRS = [(16000, 8000), (44100, 8000), (48000, 8000), (8000, 16000), (8000, 8000)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("kind,chans", [(S16, (1, 2, 32)), (Q31, (1, 2, 32)), (ULAW, (1,)), (ALAW, (1,))],
                         ids=["s16", "q31", "ulaw", "alaw"])
def test_equals_the_class_map(tfp_lib, kind, chans, pair):
    rin, rout = pair
    t = tfp_lib.resample_taps(rin, rout)
    k_hi = t["k_lo"] + t["ntaps"] - 1
    for ch in chans:
        for n in (0, 1, k_hi, k_hi + 1, 300 + ch):
            x = samples(kind, n, ch, 11 * n + ch + kind)
            # the clip a few samples into the caller's bytes: offset counts bytes
            head = samples(kind, 3, ch, 1)
            data = np.concatenate([head.reshape(-1), x.reshape(-1)])
            clip = (head.nbytes, n, rin, ch, kind, 0)
            got = tfp_lib.resample_any_pcm(data, clip, rout)
            want = class_map(tfp_lib, x, kind, rin, rout)
            assert got.dtype == np.int16 and np.array_equal(got, want), (kind, ch, n)
            assert len(got) == tfp_lib.audio_clips_check([clip], data.nbytes, rout)[0]


def test_pack_audio_clips_round_trip(tfp_lib):
    items = [(samples(ULAW, 5, 1, 1).reshape(-1), 16000), (samples(Q31, 7, 2, 2), 44100), (samples(S16, 9, 3, 3), 8000),
             (samples(ALAW, 3, 1, 4).reshape(-1), 8000, ALAW)]
    data, clips = tfp_lib.pack_audio_clips(items)
    assert list(clips["kind"]) == [ULAW, Q31, S16, ALAW] and list(clips["channels"]) == [1, 2, 3, 1]
    assert list(clips["nframes"]) == [5, 7, 9, 3] and all(int(o) % 4 == 0 for o in clips["offset"])
    for it, c in zip(items, clips):
        x = np.asarray(it[0])
        x = x.reshape(len(x), -1)
        assert np.array_equal(tfp_lib.resample_any_pcm(data, c, 8000), class_map(tfp_lib, x, int(c["kind"]), it[1], 8000))
