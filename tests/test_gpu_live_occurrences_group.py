"""tfp_live_occurrences on a device group (devices 0,0: two shards sharing the GPU): the merged rows are
offered once, every shard carries the traces of its own clips' tracks, and the selection runs on the union,
so occurrences, dropped counts and lists equal the single engine's and the composed reference's
(live_occurrence_util.Ref on a single engine beside the group), with clips on both shards and max_tracks
bounding a channel's list over the shards together."""
import pytest

import live_occurrence_util as LO
import occurrence_util as O
import test_gpu_live_occurrences as E

pytestmark = pytest.mark.gpu

NCH, WINDOW, K, GAP, HITS = E.NCH, E.WINDOW, E.K, E.GAP, E.HITS


@pytest.fixture(scope="module")
def both(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng = tfp_lib.Engine(0)
    db = LO.build_db(tfp_lib, eng)
    grp = tfp_lib.Group([0, 0])
    LO.build_db(tfp_lib, grp, fingerprinter=eng)
    yield eng, grp, db, E.calls(tfp_lib, db)
    grp.close()
    eng.close()


@pytest.mark.parametrize("max_tracks", [64, 2])
def test_group_equals_engine_and_reference(tfp_lib, both, max_tracks):
    eng, grp, db, src = both
    one = tfp_lib.Live(eng, NCH, E.FRAMES * 256)
    lv = tfp_lib.GroupLive(grp, NCH, E.FRAMES * 256)
    ref = LO.Ref(tfp_lib, eng, lv, db, own=False)
    p = tfp_lib.params(1, 0.45)
    shards, dropped = set(), 0
    step = 3 * LO.T
    for t in range(30 * 256 // step, E.FRAMES * 256 // step):
        blk = src[:, :t * step] if not one.samples(0) else src[:, (t - 1) * step:t * step]
        assert one.push(blk, None) is None and lv.push(blk, None) is None
        scopes = E.SCOPES if t % 5 else [-1, 2, 0]
        got, drop = ref.call(p, scopes, K, WINDOW, GAP, HITS, max_tracks, where=t)
        egot, edrop = one.occurrences(p, scopes, K, WINDOW, GAP, HITS, max_tracks)
        assert [O.strip(g) for g in got] == [O.strip(g) for g in egot] and drop == edrop, t
        dropped += sum(drop)
        for ch in range(NCH):
            a, b = lv.tracks(ch), one.tracks(ch)
            keys = LO.TRACK_KEYS[1:]
            assert [{q: x[q] for q in keys} for x in a] == [{q: x[q] for q in keys} for x in b], (t, ch)
            assert len(a) <= max_tracks
            shards |= {x["clip_id"] for x in a}
    assert shards == {0, 1}  # tracks of clips on both shards
    assert dropped > 0 or max_tracks == 64
    st = lv.occurrence_stats()
    assert len(st) == 2 and all(s["tracks_dropped"] == dropped for s in st)
    assert sum(s["tracks_added"] for s in st) == one.occurrence_stats()["tracks_added"]
    assert one.occurrence_stats()["retraces"] == 0 and all(s["retraces"] == 0 for s in st)  # (no stamp changes here)
    assert sum(s["frames_traced"] for s in st) == one.occurrence_stats()["frames_traced"]
    lv.reset(1)
    assert lv.tracks(1) == [] and lv.tracks(0) != []
    lv.close()
    one.close()
