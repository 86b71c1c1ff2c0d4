"""The trailing window of live calls on a device group (tfp_group_live_window): a group of 3 engines on
device 0 equals one engine call for call, both equal the scoped search of each channel's window of kept
frame values, and every shard serves every call from a window table of its own."""
import os

import numpy as np
import pytest

import live_util as L
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


def _both(tfp_lib, eng, grp, lve, lvg, hist, blk, p, scopes, k, window, where):
    """An ingest-only push on both, then the window call of each against its own owner's definition; the
    group's (uuid, count) rows equal the single engine's (clip_id differs: the group's is the shard)."""
    W.push_all(lve, [h.copy() for h in hist], blk)
    W.push_all(lvg, hist, blk)
    re_ = W.check_window(tfp_lib, eng, lve, p, scopes, k, window, where)
    rg = W.check_window(tfp_lib, grp, lvg, p, scopes, k, window, where)
    assert [R.pairs(r) for r in rg] == [R.pairs(r) for r in re_], where
    assert np.array_equal(lvg.frames(3), lve.frames(3))
    return rg


def test_group_equals_one_engine_every_tick(tfp_lib, oracle, pair):
    eng, grp, db = pair
    ticks, window, tol, k = W.TICKS, 7, 0.45, 3
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, tol)
    lve, lvg = tfp_lib.Live(eng, 8, ticks * T), tfp_lib.GroupLive(grp, 8, ticks * T)
    rows_of = W.Rows(8)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    shards = set()
    for t in range(ticks):
        rows = _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, t * T:(t + 1) * T], p, L.SCOPES8, k, window, t)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lve, t)
        shards |= {r["clip_id"] for c in range(8) for r in rows[c]}
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], tol, L.SCOPES8[c], k, window), c
    assert shards == {0, 1, 2}  # rows come from every shard
    # every shard keeps every channel: each slid its own table through the same ranges
    for st in lvg.window_stats():
        assert st == rows_of.exp
    assert all(st["incremental_pushes"] == 0 for st in lvg.stats())
    lve.close()
    lvg.close()


def test_group_tie_enrolment(tfp_lib, pair):
    eng, grp, db = pair
    window = 7
    src = L.calls(tfp_lib, db, 20 * T)
    lve, lvg = tfp_lib.Live(eng, 8, 20 * T), tfp_lib.GroupLive(grp, 8, 20 * T)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    p = tfp_lib.params(1, 0.45)
    state = {"t": 0}

    def ticks(n, why):
        for _ in range(n):
            t = state["t"]
            rows = _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, t * T:(t + 1) * T], p, L.SCOPES8, 3, window, (why, t))
            state["t"] += 1
        return rows

    first = ticks(12, "start")[0][0]
    fr = eng.fingerprint(db["pcm"][L.TWIN[0]])
    top = "ffffffff-2222-4000-8000-0000000000ff"
    for o in (eng, grp):  # a third copy of channel 0's clip under the greatest uuid: it ties with the first row, so rank 1
        o.index_add(top, fr["m1"], fr["m2"])
        o.index_set_scope([top], [2])
    rows = ticks(3, "tie enrolment")
    assert [r["audio_uuid"] for r in rows[0][:2]] == [top, first["audio_uuid"]]
    assert rows[0][0]["match_count"] == rows[0][1]["match_count"]
    for o in (eng, grp):
        o.index_remove(top)
    rows = ticks(3, "removal")
    assert rows[0][0]["audio_uuid"] == first["audio_uuid"]
    # the slid form on every shard; the shard that took the clip restarted its table for the enrolment and
    # for the removal, a shard whose index did not change kept its own
    for st in lvg.window_stats():
        assert st["general_calls"] == 0 and st["slid_calls"] == state["t"] and 1 <= st["rebuilds"] <= 3
    assert max(st["rebuilds"] for st in lvg.window_stats()) == 3 and lve.window_stats()["rebuilds"] == 3
    with pytest.raises(tfp_lib.TfpError) as ei:
        lvg.window(p, L.SCOPES8, 3, 0)
    assert ei.value.code == -1
    lve.close()
    lvg.close()
