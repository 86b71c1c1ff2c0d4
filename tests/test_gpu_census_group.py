"""Match census on a group (tfp_group_census*): three shards on device 0 equal one engine equal brute
force, with a scope split across the shards and equal counts across the shards."""
import numpy as np
import pytest

import census_util as U
import ranked_util as R
import scoped_util as S

pytestmark = pytest.mark.gpu

ANY = U.ANY
KINDS = [ANY, 0, 1, 2, S.UNUSED_SCOPE]


def test_group_of_three_equals_one_engine_equals_brute_force(engine, tfp_lib, oracle):
    scen, _ = R.load_cases()
    census = U.load_census()
    g = tfp_lib.Group([0, 0, 0])
    try:
        for name in ("rand_05", "tie_2000"):
            s = scen[name]
            n = len(s["uuids"])
            # equal clips land on the shards in turn: scopes by c // 3 % 3 spread each scope over all three shards
            scopes = [c // 3 % 3 if name == "tie_2000" else c % 3 for c in range(n)]
            for e in (engine, g):
                R.enrol(e, s)
                e.index_set_scope(s["uuids"], scopes)
            scope_of = dict(zip(s["uuids"], scopes))
            by_p = {}
            for qi, q in enumerate(s["queries"]):
                if q["coefs"] in (1, 2):
                    by_p.setdefault((q["coefs"], repr(q["tol"]), q["low"], q["high"]), []).append(qi)
            for qis in by_p.values():
                q0 = s["queries"][qis[0]]
                p = tfp_lib.params(q0["coefs"], q0["tol"], q0["low"], q0["high"])
                frames = [R.frames_from_q(s["queries"][i]["q1"], s["queries"][i]["q2"]) for i in qis for _ in KINDS]
                fr = np.concatenate(frames)
                qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
                got = g.census_batch(fr, qoff, p, KINDS * len(qis))
                assert np.array_equal(got, engine.census_batch(fr, qoff, p, KINDS * len(qis))), name
                for j, i in enumerate(qis):
                    q = s["queries"][i]
                    assert np.array_equal(got[j * 5], U.dense(census[(name, i)][0], n, got.shape[1])), (name, i)
                    for t, x in list(enumerate(KINDS))[1:] if j < 4 else ():
                        exp = U.brute_census(oracle, s["uuids"], scope_of, s["clip"], s["m1"], s["m2"], q["q1"], q["q2"],
                                             q["coefs"], q["tol"], q["low"], q["high"], x, got.shape[1])
                        assert np.array_equal(got[j * 5 + t], exp), (name, i, x)
            if name == "tie_2000":  # 2,000 equal counts in one bin, each scope's share of them summed over the shards
                assert got[0].max() == 2000 and got[1:4].max(axis=1).tolist() == [scopes.count(x) for x in range(3)]
        # the PCM form, and TFP_E_CAPACITY from every shard as from one engine
        pcm = tfp_lib.synth_pcm(0x7153A1, range(1), 16000).reshape(-1)
        a = g.census_pcm_batch(pcm, [0, 16000], tfp_lib.params(1, 0.45), [ANY])
        assert np.array_equal(a, engine.census_pcm_batch(pcm, [0, 16000], tfp_lib.params(1, 0.45), [ANY])) and a.sum() == n
        with pytest.raises(tfp_lib.TfpError) as err:
            g.census_pcm_batch(pcm, [0, 16000], tfp_lib.params(1, 0.45), [ANY], nbins=a.shape[1] - 1)
        assert err.value.code == -5
    finally:
        g.close()
        engine.index_clear()
