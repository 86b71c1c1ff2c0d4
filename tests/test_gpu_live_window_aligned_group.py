"""The aligned trailing window of live calls on a device group (tfp_group_live_window_aligned): a group of 3
engines on device 0 gives tfp_group_live_window's rows, and every kept row carries the alignment the
single engine computes for it, whichever shard holds its clip."""
import os

import numpy as np
import pytest

import live_util as L
import live_window_aligned_util as WA
import live_window_util as W
import ranked_util as R

pytestmark = pytest.mark.gpu

T = W.T


@pytest.fixture(scope="module")
def pair(tfp_lib):
    """(engine, group of 3 on device 0), the same DB in both; the index delta at this DB size too."""
    old = os.environ.get("TFP_INDEX_DELTA")
    os.environ["TFP_INDEX_DELTA"] = "1"
    try:
        if tfp_lib.device_count() < 1:
            pytest.skip("no GPU visible")
        eng, grp = tfp_lib.Engine(0), tfp_lib.Group([0, 0, 0])
    finally:
        if old is None:
            del os.environ["TFP_INDEX_DELTA"]
        else:
            os.environ["TFP_INDEX_DELTA"] = old
    db = L.build_db(tfp_lib, eng)
    L.build_db(tfp_lib, grp)
    yield eng, grp, db
    grp.close()
    eng.close()


def test_group_rows_and_alignments_equal_one_engine(tfp_lib, pair):
    eng, grp, db = pair
    ticks, window, k = 24, 7, 3
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    lve, lvg = tfp_lib.Live(eng, 8, 30 * T), tfp_lib.GroupLive(grp, 8, 30 * T)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    shards, mixed, tied = set(), 0, 0
    state = {"t": 0}

    def tick():
        nonlocal mixed, tied
        t = state["t"]
        blk = src[:, t * T:(t + 1) * T]
        W.push_all(lve, [h.copy() for h in hist], blk)
        W.push_all(lvg, hist, blk)
        re_, ae, fce, ffe = WA.check_aligned(tfp_lib, eng, lve, p, L.SCOPES8, k, window, t)
        rg, ag, fcg, ffg = lvg.window_aligned(p, L.SCOPES8, k, window)
        assert lvg.window(p, L.SCOPES8, k, window) == (rg, fcg, ffg), t  # tfp_group_live_window's rows
        assert [R.pairs(r) for r in rg] == [R.pairs(r) for r in re_] and (fcg, ffg) == (fce, ffe), t
        assert ag == ae, t  # row for row the single engine's alignments
        for c in range(8):
            ids = [r["clip_id"] for r in rg[c]]
            shards.update(ids)
            mixed += len(set(ids)) > 1
            for x, y in zip(rg[c], rg[c][1:]):
                tied += x["match_count"] == y["match_count"] and x["clip_id"] != y["clip_id"]
        state["t"] += 1
        return rg

    for _ in range(ticks):
        tick()
    # a third copy of channel 0's clip under the greatest uuid: a tie at rank 1, in the group across shards
    fr = eng.fingerprint(db["pcm"][L.TWIN[0]])
    top = "ffffffff-2222-4000-8000-0000000000ff"
    for o in (eng, grp):
        o.index_add(top, fr["m1"], fr["m2"])
        o.index_set_scope([top], [2])
    for _ in range(3):
        rows = tick()
    for o in (eng, grp):
        o.index_remove(top)
    for _ in range(3):
        rows = tick()
    assert all(r["audio_uuid"] != top for c in range(8) for r in rows[c])
    assert shards == {0, 1, 2} and mixed and tied  # clip_id is the shard; top k mixes shards, ties across them
    sts = lvg.window_aligned_stats()
    assert len(sts) == 3 and all(st["general_calls"] == 0 and st["inplace_calls"] == state["t"] for st in sts)
    with pytest.raises(tfp_lib.TfpError) as ei:
        lvg.window_aligned(p, L.SCOPES8, 3, 0)
    assert ei.value.code == -1
    lve.close()
    lvg.close()
