"""Verdicts and G.711 pushes of live calls on a device group (tfp_group_live_verdict,
tfp_group_live_push_g711): a group of 3 engines on device 0 equals one engine at every push, and both
equal the rule over the CPU oracle's counts (application_handler.c:163, :248-312; fp_handler.c:604)."""
import numpy as np
import pytest

import ranked_util as R
import verdict_util as V

pytestmark = pytest.mark.gpu

T = V.T


@pytest.fixture(scope="module")
def pair(tfp_lib, oracle):
    V.assert_data(oracle)
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng, grp = tfp_lib.Engine(0), tfp_lib.Group([0, 0, 0])
    d = V.db(oracle)
    V.enrol(eng, d)
    V.enrol(grp, d)
    yield eng, grp, d
    grp.close()
    eng.close()


def _codes(tfp_lib, pcm, law):
    table = tfp_lib.decode_g711(np.arange(256, dtype=np.uint8), law).astype(np.int32)
    order = np.argsort(table, kind="stable")
    return order[np.clip(np.searchsorted(table[order], pcm.astype(np.int32)), 0, 255)].astype(np.uint8)


def test_group_equals_one_engine_every_push(tfp_lib, oracle, pair):
    """The 8 calls as mu-law and A-law payload: verdicts and rows of the group equal one engine's at every
    push and the oracle's on the expanded samples; the leader and the rival come from different shards
    in some verdicts and from one shard in others."""
    eng, grp, d = pair
    p = tfp_lib.params(1, V.TOL)
    totals = [min(c[2], 3200) for c in V.CALLS]
    scopes = [c[1] for c in V.CALLS]
    pcms = [V.call_pcm(i)[:totals[i]] for i in range(8)]
    lve, lvg = tfp_lib.Live(eng, 8, 3200), tfp_lib.GroupLive(grp, 8, 3200)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    at = [0] * 8
    split = same = 0
    for t in range(20):
        n = [min(T, totals[c] - at[c]) for c in range(8)]
        blk = np.zeros((8, T), np.int16)
        for c in range(8):
            blk[c, :n[c]] = pcms[c][at[c]:at[c] + n[c]]
        law = (tfp_lib.ULAW, tfp_lib.ALAW)[t % 2]
        codes = _codes(tfp_lib, blk, law)
        pcm = tfp_lib.decode_g711(codes, law).reshape(8, T)
        re_ = lve.push_g711(codes, law, p, scopes, 3, n)
        rg = lvg.push_g711(codes, law, p, scopes, 3, n)
        assert [R.pairs(r) for r in rg[0]] == [R.pairs(r) for r in re_[0]] and rg[1] == re_[1], t
        for c in range(8):
            hist[c] = np.concatenate([hist[c], pcm[c, :n[c]]])
            at[c] += n[c]
        ve, vg = lve.verdict(totals, p, scopes), lvg.verdict(totals, p, scopes)
        for c in range(8):
            exp = V.verdict(oracle, d, hist[c], totals[c], V.TOL, scopes[c], V.ALIVE)
            assert V.as_oracle(ve[c]) == exp and V.as_oracle(vg[c]) == exp, (t, c)
            if vg[c]["leader"] and vg[c]["rival"]:
                if vg[c]["leader"]["clip_id"] != vg[c]["rival"]["clip_id"]:
                    split += 1
                else:
                    same += 1
    assert split and same, (split, same)  # (clip_id is the shard)
    assert all(s["general_pushes"] == 0 for s in lvg.stats())
    lve.close(), lvg.close()


def test_group_argument_errors_leave_out_untouched(tfp_lib, pair):
    eng, grp, d = pair
    lvg = tfp_lib.GroupLive(grp, 2, 1024)
    lvg.push(np.zeros((2, 300), np.int16), None)
    p = tfp_lib.params(1, V.TOL)
    for tot, pp, sc in (([299, 1024], p, None), ([1024, 1025], p, None), ([1024, 1024], tfp_lib.params(2, V.TOL), None),
                        ([1024, 1024], p, [-2, 0])):
        rc, raw = V.raw_verdict(tfp_lib, lvg, tot, pp, sc)
        assert rc == -1 and all(v.decided == 77 and v.has_leader == 77 for v in raw)
    with pytest.raises(tfp_lib.TfpError) as ei:
        lvg.push_g711(np.zeros((2, 10), np.uint8), 2, None)
    assert ei.value.code == -1 and lvg.samples(0) == 300
    assert [v["decided"] for v in lvg.verdict([300, 1024], p)] == [True, False]
    lvg.close()
