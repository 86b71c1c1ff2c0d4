"""Live calls at another rate on a group (tfp_group_live_create_rate): a group of 3 engines on device 0 gives
the results of one engine: the exact history after every push, the twin run, and the capacity refusal that
leaves every shard unchanged."""
import numpy as np
import pytest

import live_rate_util as LR
import resample_util as RU

pytestmark = pytest.mark.gpu

TFP_E_CAPACITY = -5


@pytest.fixture(scope="module")
def group(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    g = tfp_lib.Group([0, 0, 0])
    yield g
    g.close()


@pytest.mark.parametrize("pair", [(16000, 8000), (44100, 8000)])
def test_history_bit_for_bit(group, tfp_lib, pair):
    ri, ro = pair
    _, M, ntaps = RU.PAIRS[pair]
    total = 4 * ntaps + 2000
    lv = tfp_lib.GroupLive(group, 4, tfp_lib.resample_count(total, ri, ro), ro, rate_in=ri)
    assert lv.rate_info() == {"rate_in": ri, "lag_in": LR.lag_of(ri, ro)}
    src = [RU.noise(total, 11), RU.rails(total, M), RU.class_clip(1, total), np.zeros(total, np.int16)]
    call = LR.Call(tfp_lib, group, lv, ri, ro, src)
    ticks = [1, 3, ntaps - 1, ntaps, ri // 50]
    step = 0
    while min(call.at[1:]) < total and step < 200:
        t = ticks[step % len(ticks)]
        call.push([0 if (c == 0 and step % 4 == 3) else (t - c if t > 3 else t) for c in range(4)])
        call.check(step)
        step += 1
    assert min(call.at[1:]) == total
    stats = lv.rate_stats()
    assert len(stats) == 3 and stats[0] == stats[1] == stats[2] and stats[0]["samples_in"] == sum(call.at)
    lv.close()


def test_twin_object_equals_one_engine(group, engine, tfp_lib):
    """The twin run on the group (a rate object against a plain one, both on the group), and its results
    against the single engine's twin run over the same DB, clip ids (a group's are shards) aside."""
    p = tfp_lib.params(1, 0.45)
    try:
        _, src = LR.build_db16(tfp_lib, group)
        got = LR.run_twin(tfp_lib, group, lambda o, n, cap, r: tfp_lib.GroupLive(o, n, cap, 8000, r), src, p)
        LR.build_db16(tfp_lib, engine)
        one = LR.run_twin(tfp_lib, engine, lambda o, n, cap, r: tfp_lib.Live(o, n, cap, 8000, r), src, p)
    finally:
        group.index_clear()
        engine.index_clear()
    LR.assert_not_empty(got)

    def rows_only(out):  # the tracks' reserved / clip ids differ by construction; rows, counts and frames do not
        return [LR.strip(r) for r in out]
    assert rows_only(got) == rows_only(one)


def test_capacity_leaves_every_shard_unchanged(group, tfp_lib):
    ri, ro = 16000, 8000
    cap = 300
    lv = tfp_lib.GroupLive(group, 3, cap, ro, rate_in=ri)
    call = LR.Call(tfp_lib, group, lv, ri, ro, [RU.noise(2000, 31), RU.noise(2000, 32), RU.noise(2000, 33)])
    call.push([500, 600, 97])
    before = [(lv.input_samples(c), lv.samples(c)) for c in range(3)]
    s0 = lv.rate_stats()
    over = LR.n_in_for(call.at[1], cap - before[1][1] + 1, ri, ro)
    blk, _ = call.tick([10, over, 10])
    with pytest.raises(tfp_lib.TfpError) as ei:
        lv.push(blk, nsamples=[10, over, 10])
    assert ei.value.code == TFP_E_CAPACITY
    assert [(lv.input_samples(c), lv.samples(c)) for c in range(3)] == before
    assert lv.rate_stats() == s0  # no shard was told
    call.push([10, over - 2, 10])
    call.check("to the capacity")
    assert lv.samples(1) == cap
    lv.close()
