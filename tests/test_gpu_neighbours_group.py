"""Catalog neighbours on a device group (tfp_group_index_neighbours): 3 engines on device 0 give what one
engine gives, which is what the brute force gives; named clips and their neighbours lie on different
shards and equal counts occur across shards."""
import numpy as np
import pytest

import neighbour_util as N
import ranked_util as R

pytestmark = pytest.mark.gpu

M = 10**6


def _uuid(i):
    return "%08x-0000-4000-8000-%012x" % (i, i)


def test_three_shards_equal_one_engine_and_the_brute_force(tfp_lib, oracle):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    rng = np.random.default_rng(333)
    n = 60
    rows = [(rng.integers(-3, 4, 8) * M, rng.integers(-2, 3, 8) * M) for _ in range(n)]
    for i in range(0, 12):  # twelve copies of one clip: equal counts whichever shards hold them
        rows[5 * i] = (np.arange(8) * M, np.zeros(8, np.int64))
    cat = N.Catalog([_uuid(i) for i in range(n)], rows, [i % 2 for i in range(n)])
    names = [0, 5, 10, 1, 2, 59, 5]
    grp = tfp_lib.Group([0, 0, 0])
    with tfp_lib.Engine(0) as eng:
        cat.enrol(eng)
        grp.index_clear()
        for c in range(n):  # one by one: the group places each clip on the shard with the fewest rows
            grp.index_add(cat.uuids[c], cat.m1[c].astype(np.int32), cat.m2[c].astype(np.int32))
        grp.index_set_scope(cat.uuids, cat.scope)
        for coefs, tol in ((1, 0.001), (1, 0.45), (2, 0.001), (1, 9.0)):
            p = tfp_lib.params(coefs, tol)
            for k in (1, 3, 32):
                for scopes in (None, [0, 1, 0, 1, N.ANY, 0, 1]):
                    one = N.check(eng, oracle, tfp_lib, cat, names, coefs, tol, k, scopes, compose=False, align_rows=2)
                    many = grp.index_neighbours([cat.uuids[c] for c in names], p, k, scopes)
                    strip = lambda res: [(r["frame_count"], [{x: v for x, v in row.items() if x != "clip_id"}
                                                             for row in r["neighbours"]]) for r in res]
                    assert strip(many) == strip(one), (coefs, tol, k, scopes)
                    shards = {row["clip_id"] for r in many for row in r["neighbours"]}
                    if k == 32 and scopes is None:
                        assert shards == {0, 1, 2}
        # the group's counters mean what the engine's do: a clip's rows read once, every returned row aligned once
        p, uu = tfp_lib.params(1, 0.45), [cat.uuids[c] for c in names]
        e0, g0 = eng.neighbour_stats(), grp.neighbour_stats()
        rows = sum(len(r["neighbours"]) for r in eng.index_neighbours(uu, p, 3))
        grp.index_neighbours(uu, p, 3)
        e1, g1 = eng.neighbour_stats(), grp.neighbour_stats()
        for key, want in (("frames_read", 8 * len(names)), ("pairs_aligned", rows)):
            assert e1[key] - e0[key] == g1[key] - g0[key] == want, (key, e0, e1, g0, g1)
        assert g1["general_batches"] - g0["general_batches"] == 3 and e1["vote_batches"] - e0["vote_batches"] == 1
    grp.close()
