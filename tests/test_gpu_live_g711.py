"""G.711 pushes of a live call (tfp_live_push_g711, live_scatter_g711_kernel in csrc/tfp_live.hip): the
rows, counts, frame counts and verdicts equal those of tfp_live_push on tfp_g711_decode(codes), bit for
bit (aubio_source's table[code], fp_handler.c:604, :633; record_voice, application_handler.c:248-312)."""
import numpy as np
import pytest

import live_util as L

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_CAPACITY = -1, -5


@pytest.fixture(scope="module")
def db(engine, tfp_lib):
    d = L.build_db(tfp_lib, engine)
    yield d
    engine.index_clear()


def _codes(tfp_lib, pcm, law):
    """Codes whose expansion is near pcm: the nearest of the law's 256 values per sample."""
    table = tfp_lib.decode_g711(np.arange(256, dtype=np.uint8), law).astype(np.int32)
    order = np.argsort(table, kind="stable")
    pos = np.clip(np.searchsorted(table[order], pcm.astype(np.int32)), 0, 255)
    return order[pos].astype(np.uint8)


@pytest.mark.parametrize("tick", [1, 3, 160, 161])
def test_pushes_equal_int16_pushes_of_the_expansion(engine, tfp_lib, db, tick):
    """Both laws and int16 interleaved within one call, ragged nsamples (0 among them), odd s_old, hop
    edges crossed: after every push the rows equal a second live object's, fed the expansion."""
    nch = 4
    total = {1: 300, 3: 600, 160: 160 * 14, 161: 161 * 14}[tick]
    src = L.calls(tfp_lib, db, total)[:nch]
    p = tfp_lib.params(1, 0.45)
    scopes = L.SCOPES8[:nch]
    a, b = tfp_lib.Live(engine, nch, total), tfp_lib.Live(engine, nch, total)
    hist = [np.zeros(0, np.int16) for _ in range(nch)]
    at = [0] * nch
    step = 0
    while any(x < total for x in at):
        # channel c takes tick - (step + c) % 3 samples where it can (so s_old goes odd and the channels drift apart), channel 0 idles every 4th push
        n = [max(0, min(total - at[c], tick - (step + c) % 3 if tick > 2 else tick)) for c in range(nch)]
        if step % 4 == 3:
            n[0] = 0
        law = (tfp_lib.ULAW, tfp_lib.ALAW, None)[step % 3]
        blk = np.zeros((nch, tick), np.int16)
        for c in range(nch):
            blk[c, :n[c]] = src[c, at[c]:at[c] + n[c]]
        search = step % 5 == 4 or tick >= 160
        if law is None:
            got = a.push(blk, p if search else None, scopes, 3, n)
            pcm = blk
        else:
            codes = _codes(tfp_lib, blk, law)
            got = a.push_g711(codes, law, p if search else None, scopes, 3, n)
            pcm = tfp_lib.decode_g711(codes, law).reshape(nch, tick)
        exp = b.push(pcm, p if search else None, scopes, 3, n)
        assert got == exp, (step, law)
        for c in range(nch):
            hist[c] = np.concatenate([hist[c], pcm[c, :n[c]]])
            at[c] += n[c]
        step += 1
    assert [a.samples(c) for c in range(nch)] == [len(h) for h in hist]
    rows = L.check_push(tfp_lib, engine, a, hist, np.zeros((nch, 1), np.int16), p, scopes, 3, nsamples=[0] * nch, where="end")
    assert any(rows)
    tot = [len(h) for h in hist]
    assert a.verdict(tot, p, scopes) == b.verdict(tot, p, scopes)
    a.close(), b.close()


@pytest.mark.parametrize("law", ["ULAW", "ALAW"])
def test_all_256_codes_in_one_tick(engine, tfp_lib, db, law):
    law = getattr(tfp_lib, law)
    codes = np.stack([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1).astype(np.uint8)])
    before = engine.g711_stats()
    a = tfp_lib.Live(engine, 2, 513)
    a.push(np.full((2, 1), 7, np.int16), None)  # s_old = 1: the tick lands at odd addresses and crosses the hop edge
    p = tfp_lib.params(1, 0.45)
    rows, fc = a.push_g711(codes, law, p, None, 2)
    hist = [np.concatenate([[7], tfp_lib.decode_g711(codes[c], law)]).astype(np.int16) for c in range(2)]
    assert fc == [2, 2] and rows == L.prefix_rows(engine, hist, p, [-1, -1], 2)
    # the kept samples themselves: coefs = 2 reads the second value of every frame
    p2 = tfp_lib.params(2, 0.1)
    assert a.push_g711(codes, law, p2, None, 2, nsamples=[0, 0])[0] == L.prefix_rows(engine, hist, p2, [-1, -1], 2)
    after = engine.g711_stats()
    assert after["stream_launches"] - before["stream_launches"] == 2 and after["codes"] - before["codes"] == 512
    a.close()


def test_bad_law_and_capacity_ingest_nothing(engine, tfp_lib, db):
    a = tfp_lib.Live(engine, 3, 400)
    codes = np.zeros((3, 160), np.uint8)
    a.push_g711(codes, tfp_lib.ULAW, None)
    for law in (-1, 2, 7):
        with pytest.raises(tfp_lib.TfpError) as ei:
            a.push_g711(codes, law, None)
        assert ei.value.code == TFP_E_ARG
    a.push_g711(codes, tfp_lib.ALAW, None, nsamples=[160, 0, 80])
    with pytest.raises(tfp_lib.TfpError) as ei:  # channel 0 would pass 400: nothing for any channel
        a.push_g711(codes, tfp_lib.ALAW, tfp_lib.params(1, 0.45), None, 1, nsamples=[81, 10, 10])
    assert ei.value.code == TFP_E_CAPACITY
    assert [a.samples(c) for c in range(3)] == [320, 160, 240]
    a.close()
