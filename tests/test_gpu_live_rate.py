"""Live calls at another rate (tfp_live_create_rate, csrc/tfp_live_rate.hip): every push is converted to the
index's rate on the GPU with a carried input tail per channel. After every push a channel's history is exactly
the first N(S_in) = resample_count(S_in - k_hi) samples of tfp_resample_pcm of its input so far (read through
its kept frames, bit for bit), and the object behaves as a plain live object that was pushed each tick's newly
settled samples."""
import numpy as np
import pytest

import live_rate_util as LR
import resample_util as RU

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
PAIRS = [(16000, 8000), (48000, 8000), (8000, 16000), (44100, 8000), (11025, 8000)]


def _live(tfp):
    return lambda owner, nch, cap, rate_in, rate_out=8000: tfp.Live(owner, nch, cap, rate_out, rate_in)


@pytest.fixture(scope="module")
def db16(engine, tfp_lib):
    d = LR.build_db16(tfp_lib, engine)
    yield d
    engine.index_clear()


def _sources(n, M):
    return [RU.noise(n, 11), RU.rails(n, M), RU.class_clip(1, n), np.zeros(n, np.int16)]


@pytest.mark.parametrize("pair", PAIRS)
def test_history_bit_for_bit(engine, tfp_lib, pair):
    """4 channels (noise, full-scale rails, a class clip, silence), ticks of 1, 3, ntaps - 1, ntaps and one
    20 ms frame in turn, ragged so that the channels drift apart, channel 0 idle every 4th push: after every
    push the settled count and the kept frames are the definition's."""
    ri, ro = pair
    _, M, ntaps = RU.PAIRS[pair]
    total = 4 * ntaps + 2000
    lv = tfp_lib.Live(engine, 4, tfp_lib.resample_count(total, ri, ro), ro, rate_in=ri)
    assert lv.rate_info() == {"rate_in": ri, "lag_in": LR.lag_of(ri, ro)}
    call = LR.Call(tfp_lib, engine, lv, ri, ro, _sources(total, M))
    ticks = [1, 3, ntaps - 1, ntaps, ri // 50]
    step = 0
    while min(call.at[1:]) < total and step < 200:
        t = ticks[step % len(ticks)]
        call.push([0 if (c == 0 and step % 4 == 3) else (t - c if t > 3 else t) for c in range(4)])
        for c in range(4):
            assert lv.samples(c) == tfp_lib.resample_count(call.at[c] - LR.lag_of(ri, ro), ri, ro), (step, c)
        call.check(step)
        step += 1
    assert min(call.at[1:]) == total and call.at[0] > 2 * ntaps
    lv.close()


@pytest.mark.parametrize("coefs,tol", [(1, 0.45), (2, 0.1)])
def test_twin_object(engine, tfp_lib, db16, coefs, tol):
    """A rate object equals a plain object pushed each step's newly settled samples: push rows and frame
    counts, window, window_aligned, occurrences and, after finish, the verdict. The calls play the 16 kHz
    sources of enrolled clips from offsets that are multiples of 256 M, so frames coincide and rows exist."""
    _, src = db16
    out = LR.run_twin(tfp_lib, engine, _live(tfp_lib), src, tfp_lib.params(coefs, tol))
    LR.assert_not_empty(out)


@pytest.mark.parametrize("pair", [(8000, 16000), (16000, 8000)])
def test_g711_pushes_interleave(engine, tfp_lib, db16, pair):
    """mu-law, A-law and int16 pushes of one call in turn on one object, their decode_g711 as int16 on another:
    equal rows, counts and kept frames after every push; all 256 codes in one tick right after a 1-sample push."""
    ri, ro = pair
    p = tfp_lib.params(1, 0.45)
    a, b = tfp_lib.Live(engine, 3, 4000, ro, rate_in=ri), tfp_lib.Live(engine, 3, 4000, ro, rate_in=ri)
    rng = np.random.default_rng(711)
    g0 = engine.g711_stats()
    plan = [(1, 0), (256, 1), (97, None), (49, 0), (160, 1), (3, None), (320, 0), (255, 1)]
    for i, (n, law) in enumerate(plan):
        ns = [n, max(n - 1, 0), n if i % 3 else 0]
        if law is None:
            blk = rng.integers(-32768, 32768, (3, n)).astype(np.int16)
            ra, dec = a.push(blk, p, nsamples=ns, k=3), blk
        else:
            codes = rng.integers(0, 256, (3, n)).astype(np.uint8)
            if n == 256:
                codes[0], codes[1] = np.arange(256), np.arange(255, -1, -1)
            ra = a.push_g711(codes, law, p, nsamples=ns, k=3)
            dec = np.stack([tfp_lib.decode_g711(codes[c], law) for c in range(3)])
        rb = b.push(dec, p, nsamples=ns, k=3)
        assert ra == rb, (i, ra, rb)
        for c in range(3):
            assert a.samples(c) == b.samples(c) and a.input_samples(c) == b.input_samples(c), (i, c)
            RU.bits_equal(a.frames(c, 0), b.frames(c, 0))
    assert a.samples(0) == tfp_lib.resample_count(sum(n for n, _ in plan) - LR.lag_of(ri, ro), ri, ro) > 256
    assert engine.g711_stats() != g0  # the code pushes were counted
    a.close()
    b.close()


def test_reset_idle_and_carry(engine, tfp_lib):
    """A call that ends in full-scale rails, then reset and a new call: no carried sample leaks. A channel
    idle for 5 pushes while the others advance, then resumed. A channel with 0 < S_in <= k_hi: carry only."""
    ri, ro = 16000, 8000
    lag = LR.lag_of(ri, ro)
    n = 1500
    lv = tfp_lib.Live(engine, 3, n, ro, rate_in=ri)
    loud = np.full((3, 400), 32767, np.int16)
    lv.push(loud, nsamples=[400, 0, 0])
    lv.push(loud, nsamples=[1, 0, 0])
    assert lv.samples(0) > 0
    lv.reset(0)
    assert lv.samples(0) == 0 and lv.input_samples(0) == 0
    call = LR.Call(tfp_lib, engine, lv, ri, ro, [RU.noise(n, 5), RU.noise(n, 6), RU.noise(n, 7)])
    call.push([3, 3, 3])
    call.check("3 after reset")
    call.push([60, 60, lag - 3])  # channel 2: S_in = lag = k_hi
    call.check("carry only")
    assert lv.input_samples(2) == lag and lv.samples(2) == 0 and len(lv.frames(2, 0)) == 0
    rows, fc = lv.push(np.zeros((3, 1), np.int16), tfp_lib.params(1, 0.45), nsamples=[0, 0, 0])
    assert rows[2] == [] and fc[2] == 0
    for i in range(5):  # channel 1 idle
        call.push([97 + i, 0, 1])
        call.check(("idle", i))
    assert lv.samples(2) > 0
    call.push([200, 200, 200])
    call.check("resumed")
    call.push([5, 97, 96])
    call.check("after")
    lv.close()


@pytest.mark.parametrize("pair", [(16000, 8000), (256000, 8000)])
def test_several_tiles_in_one_push(engine, tfp_lib, pair):
    """One push settles 2 tiles + 1 outputs on one channel, 1 on another and none on a third (n_in < lag):
    exact histories, one launch, the exact samples in and out. 256000 -> 8000: the staged-span limit makes the
    tile shorter than kRsTile (30720 - ntaps - 1 input samples, M = 32 of them per output)."""
    ri, ro = pair
    L_, M, _, k_hi = RU.plan(ri, ro)
    ntaps = k_hi + (24 * max(L_, M)) // L_ + 1
    tile = min(RU.TILE, 1 + ((RU.TILE * 30 - ntaps) * L_ - 1) // M)  # kRsTile * 30 = 30720
    assert (tile == RU.TILE) == (pair == (16000, 8000))
    first = [lag_plus for lag_plus in (k_hi + 7, k_hi + 2, 5)]
    want = [LR.n_in_for(first[0], 2 * tile + 1, ri, ro), LR.n_in_for(first[1], 1, ri, ro), k_hi - 5 - 1]
    assert None not in want
    total = [f + w for f, w in zip(first, want)]
    lv = tfp_lib.Live(engine, 3, 2 * tile + 64, ro, rate_in=ri)
    call = LR.Call(tfp_lib, engine, lv, ri, ro, [RU.noise(total[0], 21), RU.rails(total[1], M), RU.noise(total[2], 23)])
    call.push(first)
    call.check("first")
    s0 = lv.rate_stats()
    old = [lv.samples(c) for c in range(3)]
    call.push(want)
    call.check("tiles")
    new = [lv.samples(c) for c in range(3)]
    assert [n - o for n, o in zip(new, old)] == [2 * tile + 1, 1, 0]
    s1 = lv.rate_stats()
    assert s1["launches"] - s0["launches"] == 1
    assert s1["samples_in"] - s0["samples_in"] == sum(want) and s1["samples_out"] - s0["samples_out"] == 2 * tile + 2
    lv.close()


def test_capacity_and_refusals(engine, tfp_lib):
    ri, ro = 16000, 8000
    cap = 300
    lv = tfp_lib.Live(engine, 3, cap, ro, rate_in=ri)
    call = LR.Call(tfp_lib, engine, lv, ri, ro, [RU.noise(2000, 31), RU.noise(2000, 32), RU.noise(2000, 33)])
    call.push([500, 600, 97])
    before = [(lv.input_samples(c), lv.samples(c)) for c in range(3)]
    over = LR.n_in_for(call.at[1], cap - before[1][1] + 1, ri, ro)
    blk, _ = call.tick([10, over, 10])
    for p in (None, tfp_lib.params(1, 0.45)):
        with pytest.raises(tfp_lib.TfpError) as ei:
            lv.push(blk, p, nsamples=[10, over, 10])
        assert ei.value.code == TFP_E_CAPACITY
        assert [(lv.input_samples(c), lv.samples(c)) for c in range(3)] == before
    call.push([10, over - 2, 10])  # exactly to the capacity (M = 2: two samples fewer settle one output fewer)
    call.check("to the capacity")
    assert lv.samples(1) == cap
    lv.close()
    for args, msg in (((0, 8000), "bad sample rate"), ((7999, 44100), "unsupported rate ratio"),
                      ((5600000, 8000), "unsupported rate ratio")):
        with pytest.raises(tfp_lib.TfpError) as ei:
            tfp_lib.Live(engine, 2, 1000, args[1], rate_in=args[0])
        assert ei.value.code == TFP_E_ARG and msg in str(ei.value), (args, str(ei.value))
    # equal rates: a plain object
    a, b = tfp_lib.Live(engine, 2, 2000, 8000, rate_in=8000), tfp_lib.Live(engine, 2, 2000, 8000)
    assert a.rate_info() == {"rate_in": 8000, "lag_in": 0} == b.rate_info()
    p = tfp_lib.params(1, 0.45)
    x = np.stack([RU.noise(900, 41), RU.class_clip(0, 900)])
    for at in (0, 300, 600):
        assert a.push(x[:, at:at + 300], p, k=3) == b.push(x[:, at:at + 300], p, k=3)
    a.finish()
    assert [a.samples(c) for c in range(2)] == [900, 900] == [a.input_samples(c) for c in range(2)]
    assert a.rate_stats() == {"launches": 0, "samples_in": 0, "samples_out": 0}
    for c in range(2):
        RU.bits_equal(a.frames(c, 0), b.frames(c, 0))
    a.close()
    b.close()


@pytest.mark.parametrize("pair", [(48000, 8000), (8000, 16000)])
def test_finish(engine, tfp_lib, pair):
    """After finish every output is settled: samples = resample_count(S_in), the frames are those of the whole
    resample_pcm, and a verdict planned for that many samples is complete."""
    ri, ro = pair
    _, M, ntaps = RU.PAIRS[pair]
    n = [2 * ntaps + 700, 2 * ntaps + 333, 40]
    lv = tfp_lib.Live(engine, 3, 4000, ro, rate_in=ri)
    call = LR.Call(tfp_lib, engine, lv, ri, ro, [RU.noise(n[0], 51), RU.rails(n[1], M), RU.noise(n[2], 53)])
    while call.at != n:
        call.push([ri // 50] * 3)
    call.check("before")
    lv.finish()
    for c in range(3):
        assert lv.samples(c) == tfp_lib.resample_count(n[c], ri, ro)
    call.at = [k + LR.lag_of(ri, ro) for k in n]
    call.src = [np.concatenate([x, np.zeros(LR.lag_of(ri, ro), np.int16)]) for x in call.src]
    for c in range(3):  # the flushed history is the call's own resample_pcm, last outputs included
        assert np.array_equal(call.expected(c), tfp_lib.resample_pcm(call.src[c][:n[c]], ri, ro))
    call.check("finished")
    v = lv.verdict([lv.samples(c) for c in range(3)], tfp_lib.params(1, 0.45))
    assert all(x["complete"] for x in v)
    lv.close()
