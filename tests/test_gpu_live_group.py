"""Live calls on a device group (tfp_group_live_*): a group of 3 engines on device 0 equals one
engine tick for tick, and both equal the scoped search of each call so far; ties cross shards (the
twin clips' rows merge by uuid whichever shards hold them)."""
import numpy as np
import pytest

import live_util as L
import ranked_util as R

pytestmark = pytest.mark.gpu

T = 160


@pytest.fixture(scope="module")
def pair(tfp_lib):
    """(engine, group of 3 on device 0), the same DB in both; the index delta at this DB size too."""
    import os
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


def _both(tfp_lib, eng, grp, lve, lvg, hist, blk, p, scopes, k, nsamples=None, where=None):
    """The push on the group checked against the group's own prefix search, and its (uuid, count) rows
    against the single engine's push (clip_id differs: the group's is the shard)."""
    he = [h.copy() for h in hist]
    re_ = L.check_push(tfp_lib, eng, lve, he, blk, p, scopes, k, nsamples, where)
    rg = L.check_push(tfp_lib, grp, lvg, hist, blk, p, scopes, k, nsamples, where)
    assert [R.pairs(r) for r in rg] == [R.pairs(r) for r in re_], where
    return rg


def test_group_equals_one_engine_every_tick(tfp_lib, oracle, pair):
    eng, grp, db = pair
    ticks = 20
    src = L.calls(tfp_lib, db, ticks * T)
    shards = set()
    for tol, k in ((0.001, 1), (0.45, 3), (0.45, 32)):
        p = tfp_lib.params(1, tol)
        lve, lvg = tfp_lib.Live(eng, 8, ticks * T), tfp_lib.GroupLive(grp, 8, ticks * T)
        hist = [np.zeros(0, np.int16) for _ in range(8)]
        for t in range(ticks):
            rows = _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, t * T:(t + 1) * T], p, L.SCOPES8, k, where=(tol, k, t))
        for c in range(8):
            assert R.pairs(rows[c]) == L.oracle_rows(oracle, db, hist[c], tol, L.SCOPES8[c], k), c
        shards |= {r["clip_id"] for c in range(8) for r in rows[c]}
        for st in lvg.stats() + [lve.stats()]:
            assert st["incremental_pushes"] == ticks and st["general_pushes"] == 0 and st["rebuilds"] == 1
        lve.close()
        lvg.close()
    assert shards == {0, 1, 2}  # rows come from every shard


def test_group_hop_edges_and_capacity(tfp_lib, pair):
    eng, grp, db = pair
    sizes = [1000, 1, 255, 256, 257, 511, 512, 513]
    src = L.calls(tfp_lib, db, sum(sizes))
    p = tfp_lib.params(1, 0.45)
    lve, lvg = tfp_lib.Live(eng, 8, sum(sizes)), tfp_lib.GroupLive(grp, 8, sum(sizes))
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    at = [0] * 8
    for tk in sizes:
        n = [tk * c // 7 for c in range(8)]
        blk = np.zeros((8, tk), np.int16)
        for c in range(8):
            blk[c, :n[c]] = src[c, at[c]:at[c] + n[c]]
            at[c] += n[c]
        _both(tfp_lib, eng, grp, lve, lvg, hist, blk, p, L.SCOPES8, 3, nsamples=n, where=tk)
    # channel 7 is full: a capacity failure leaves every shard unchanged
    before = [lvg.samples(c) for c in range(8)]
    with pytest.raises(tfp_lib.TfpError) as ei:
        lvg.push(src[:, :1], p, L.SCOPES8, 3)
    assert ei.value.code == -5
    assert [lvg.samples(c) for c in range(8)] == before
    _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, :1], p, L.SCOPES8, 3, nsamples=[0] * 8, where="after capacity")
    lvg.reset()
    lve.reset()
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, :254], p, L.SCOPES8, 3, where=254)
    for i in range(254, 258):
        _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, i:i + 1], p, L.SCOPES8, 3, where=i + 1)
    assert all(st["general_pushes"] == 0 and st["rebuilds"] == 1 for st in lvg.stats())
    lve.close()
    lvg.close()


def test_group_mid_call_changes(tfp_lib, pair):
    eng, grp, db = pair
    src = L.calls(tfp_lib, db, 30 * T)
    lve, lvg = tfp_lib.Live(eng, 8, 30 * T), tfp_lib.GroupLive(grp, 8, 30 * T)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    state = {"t": 0, "p": tfp_lib.params(1, 0.45), "scopes": list(L.SCOPES8)}

    def ticks(n, why):
        for _ in range(n):
            t = state["t"]
            rows = _both(tfp_lib, eng, grp, lve, lvg, hist, src[:, t * T:(t + 1) * T], state["p"], state["scopes"], 3,
                         where=(why, t))
            state["t"] += 1
        return rows

    first = ticks(8, "start")[0][0]
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
    for o in (eng, grp):
        o.index_commit()
    ticks(2, "commit")
    state["p"] = tfp_lib.params(1, 0.001, 3, 2000)
    ticks(3, "tolerance and ignore filter")
    state["scopes"] = [-1, 2, 0, 1, 7, 0, 2, -1]
    ticks(3, "scopes")
    state["p"] = tfp_lib.params(2, 0.1)
    ticks(2, "coefs 2")
    assert all(st["general_pushes"] == 2 and st["incremental_pushes"] == state["t"] - 2 for st in lvg.stats())
    lve.close()
    lvg.close()
