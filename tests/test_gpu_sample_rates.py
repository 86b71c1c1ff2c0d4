"""Fingerprints at every sample-rate class, bit for bit against the CPU oracle at the same rate.

build_tables (csrc/tfp_tables.cpp) derives from the rate everything the kernels read: the sparse
filters, the 3 x 16 slot schedule with its slot-2 log deferral, and the frame-pair schedule that
decides (DspTables_fixed8k) whether the 8 kHz kernels run. RATES holds one rate per shape of those
tables (tests/test_tables.py CLASS_SHAPES pins the shapes on the host); each goes through every
fingerprint entry point, with the kernel that ran asserted from the launch counter. Stored
micro-units and the q doubles are compared exactly, NULLs included: no tolerance anywhere."""
import numpy as np
import pytest

from fp_util import assert_frames_equal, assert_only_kernel
from g711_util import ALAW, ULAW, encode, expand
from test_gpu_parity import _sparse_cases

pytestmark = pytest.mark.gpu

RATES = [1, 100, 500, 1000, 2000, 4000, 6000, 7999, 8001, 11025, 12000, 22050, 32000, 48000, 96000, 192000, 1000000]

# 7999 and 8001 Hz take the 8 kHz kernel family, and rightly so. DspTables_fixed8k (tfp_kernels.hip)
# asks for the shape the kernels fix at compile time, not for the rate: slots of 36 / 16 / 8 bins in
# 960 floats of LDS, deferral on, a frame-pair schedule of kFbNf = 34 filters with the 6 empty ones
# above them. Everything else fingerprint8k_kernel uses it reads from the tables it is handed:
# window_s, twiddles, ms_filter / ms_start / ms_w (small launch), fb_bin / fb_new / fb_filter / fb_w
# (throughput launch), ms_c_real, mel_len for the empty filters' constant, the DCT rows. The tables
# of 7997..8020 Hz (and 7954..7959) have that shape with their own weights and lane order
# (test_tables.py::test_slot_schedule_sweep), so the exact comparison below proves the fixed kernels
# on weights that are not the 8 kHz ones.
FIXED_SHAPE = (7999, 8001)
# ms_total (1920 and 1152 floats, CLASS_SHAPES) > kMsLds = 960 (tfp_kernels.hip): fingerprint_kernel
# leaves the slot weights in global memory and mel3 runs over T->ms_w.
GLOBAL_WEIGHTS = (500, 1000)
ALL_EMPTY = (1, 100)  # every filter empty: c0 a constant, c1 a cancellation residue

LENGTHS = [0, 1, 255, 256, 257, 513, 4097]
KINDS = ["synth", "silence", "altfull", "tiny"]
SEED = 0x5A3E


def _clip(tfp_lib, rng, kind, n, i):
    if kind == "silence":
        return np.zeros(n, np.int16)
    if kind == "altfull":
        return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "tiny":
        return rng.integers(-2, 3, n).astype(np.int16)
    return tfp_lib.synth_pcm(SEED, [i], n)[0] if n else np.zeros(0, np.int16)


class Inputs:
    pass


@pytest.fixture(scope="module")
def inputs(tfp_lib):
    """The ragged set (every length twice, so that each of the two longest meets two kinds) and the
    320-clip batch (sparse and cancelling spectra, synthetic audio, full-scale noise); host only."""
    rng = np.random.default_rng(0x5A)
    x = Inputs()
    x.clips = [_clip(tfp_lib, rng, KINDS[(i + 2 * (i // len(LENGTHS))) % 4], n, i) for i, n in enumerate(LENGTHS * 2)]
    assert [len(c) for c in x.clips] == LENGTHS * 2
    x.flat = np.concatenate(x.clips)
    x.off = np.concatenate([[0], np.cumsum([len(c) for c in x.clips])]).astype(np.int64)
    big = _sparse_cases(nclips=320)
    synth = tfp_lib.synth_pcm(SEED, range(80), 4096)
    for i in range(0, 320, 4):
        big[i] = synth[i // 4]
        big[i + 1] = rng.integers(-32768, 32768, 4096).astype(np.int16)
    x.big = np.concatenate(big)
    x.big_off = (np.arange(321) * 4096).astype(np.int64)
    # fp32 hop values: the ragged clips as s / 32768 (exact), every other one scaled off the int16 grid
    x.f32 = [c.astype(np.float32) / np.float32(32768) * np.float32(1.0 if i % 2 else 0.7391) for i, c in enumerate(x.clips)]
    # and non-finite samples (a float WAV may hold them): aubio's dense filterbank makes every band of
    # such a frame NaN (0 * inf), empty filters included, so these frames are NULL at every rate; the
    # kernel redoes them from the sparse filters (mel_start / mel_len / mel_off / mel_w)
    base = (0.3 * np.sin(2 * np.pi * 0.0875 * np.arange(4097 + 300))).astype(np.float32)
    bad = base.copy()
    bad[700], bad[2000], bad[2001] = np.inf, -np.inf, np.nan
    huge = (base * np.float32(3e38)).astype(np.float32)  # the FFT's sums overflow
    x.f32 += [bad, huge]
    x.f32_off = np.concatenate([[0], np.cumsum([len(c) for c in x.f32])]).astype(np.int64)
    x.codes = {law: [encode(c, law) for c in x.clips] for law in (ULAW, ALAW)}
    return x


def _oracle_clips(oracle, clips, sr, f32=False):
    want = [(oracle.fingerprint_f32 if f32 else oracle.fingerprint)(c, sr) for c in clips]
    return np.concatenate([w[2] for w in want]), np.concatenate([w[1] for w in want])


@pytest.mark.parametrize("sr", RATES)
def test_fingerprint_paths_bit_exact(engine, oracle, inputs, sr):
    x = inputs
    fixed = sr in FIXED_SHAPE
    i16_small, i16_batch = ("small8k", "throughput8k") if fixed else ("generic_i16", "generic_i16")

    micro, db = _oracle_clips(oracle, x.clips, sr)
    if sr in GLOBAL_WEIGHTS:
        from test_tables import CLASS_SHAPES
        assert CLASS_SHAPES[sr][1] > 960  # (test_slot_schedule_class_rates reads it off build_tables)
    fmicro, fdb = _oracle_clips(oracle, x.f32, sr, f32=True)
    if sr in ALL_EMPTY:
        # From the oracle alone, so that the case cannot pass vacuously. With every filter empty each
        # band log is the constant log10 of the clamped 0, c0 = -263.728 and c1 is the DCT row's
        # cancellation residue, -9.5367e-07: not 0, so int16 audio gives the one finite pair
        # (24.211562, -60.205999) in every frame and never a NULL. The NULL rule is reached at these
        # rates by the fp32 clips with non-finite samples, whose frames are NaN in every band.
        assert (micro == micro[0]).all() and tuple(micro[0]) == (24211562, -60205999) and np.isfinite(db).all()
        assert (fmicro[:, 1] == oracle.NULL_MICRO).any() and (~np.isfinite(fdb[:, 1])).any()
        assert (fmicro[:, 1] == -60205999).any()

    # single clips: the small launch
    st = engine.fingerprint_stats()
    foff = np.concatenate([[0], np.cumsum((np.diff(x.off) + 255) // 256)])
    for c, clip in enumerate(x.clips):
        fr = engine.fingerprint(clip, sr)
        assert_frames_equal(fr, micro[foff[c]:foff[c + 1]], db[foff[c]:foff[c + 1]])
        assert np.array_equal(fr["frame_idx"], np.arange(len(fr)))
    assert_only_kernel(engine, st, i16_small)

    # the 320-clip batch: past the small launch's size
    bmicro, bdb = oracle.fingerprint_batch(x.big, x.big_off, sr, nthreads=8)
    st = engine.fingerprint_stats()
    fr = engine.fingerprint_batch(x.big, x.big_off, sr)
    assert_only_kernel(engine, st, i16_batch, "the batch became a small one: add clips")
    assert_frames_equal(fr, bmicro, bdb)

    # fp32 samples
    assert (fmicro == oracle.NULL_MICRO).any()
    st = engine.fingerprint_stats()
    fr = engine.fingerprint_f32_batch(np.concatenate(x.f32), x.f32_off, sr)
    assert_only_kernel(engine, st, "generic_f32")
    assert_frames_equal(fr, fmicro, fdb)

    # G.711 codes, both laws, on the ragged set
    for law in (ULAW, ALAW):
        gmicro, gdb = _oracle_clips(oracle, [expand(c, law) for c in x.codes[law]], sr)
        st = engine.fingerprint_stats()
        fr = engine.fingerprint_g711_batch(np.concatenate(x.codes[law]), x.off, law, sr)
        assert_only_kernel(engine, st, i16_small)
        assert_frames_equal(fr, gmicro, gdb)

    # the device-plan form, once (a plan always takes the throughput launch of its kernel family)
    torch = pytest.importorskip("torch")
    buf = torch.from_numpy(x.flat).cuda()
    plan = engine.plan(x.off, sr)
    assert plan.nframes == len(micro)
    dm = torch.zeros((plan.nframes, 2), dtype=torch.int32, device="cuda")
    dq = torch.zeros((plan.nframes, 2), dtype=torch.float64, device="cuda")
    st = engine.fingerprint_stats()
    engine.fingerprint_device(plan, buf.data_ptr(), dm.data_ptr(), dq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_only_kernel(engine, st, i16_batch)
    m, q = dm.cpu().numpy(), dq.cpu().numpy()
    fr = np.zeros(plan.nframes, [("m1", "<i4"), ("m2", "<i4"), ("q1", "<f8"), ("q2", "<f8")])
    fr["m1"], fr["m2"], fr["q1"], fr["q2"] = m[:, 0], m[:, 1], q[:, 0], q[:, 1]
    assert_frames_equal(fr, micro, db)


@pytest.mark.parametrize("sr", [4000, 48000])
def test_stream_and_live_at_other_rates(engine, oracle, tfp_lib, sr):
    """A stream's window and a live call's frames after uneven pushes equal the oracle's fingerprint
    of the same samples at the stream's rate."""
    from tiresias_amd import Live, Stream
    W, nch = 4001, 2
    ticks = [1000, 1, 2999, 257, 513, 4001, 160, 255]
    total = sum(ticks)
    rng = np.random.default_rng(sr)
    src = np.stack([tfp_lib.synth_pcm(SEED, [3], total)[0], rng.integers(-32768, 32768, total).astype(np.int16)])
    stm, lv = Stream(engine, nch, W, sample_rate=sr), Live(engine, nch, total, sample_rate=sr)
    st0 = engine.fingerprint_stats()
    pos = checked = 0
    try:
        for T in ticks:
            blk = src[:, pos:pos + T]
            pos += T
            assert stm.push(blk) is None
            assert lv.push(blk) is None
            for c in range(nch):
                fr = stm.window_frames(c)
                if pos < W:
                    assert len(fr) == 0
                else:
                    _, db, micro = oracle.fingerprint(src[c, pos - W:pos], sr)
                    assert_frames_equal(fr, micro, db)
                    checked += 1
                _, db, micro = oracle.fingerprint(src[c, :pos], sr)
                assert lv.samples(c) == pos
                assert_frames_equal(lv.frames(c), micro, db)
    finally:
        stm.close()
        lv.close()
    assert checked >= 2 * 4
    assert_only_kernel(engine, st0, "generic_i16")


@pytest.mark.parametrize("sr", [11025, 48000])
def test_search_pcm_at_other_rates(engine, oracle, tfp_lib, sr):
    """search_pcm_batch at the index's own rate == search_batch on the oracle-checked frames of the
    same queries == the oracle's search, against 6 clips enrolled at that rate."""
    nclips, n = 6, 256 * 60
    pcm = tfp_lib.synth_pcm(SEED, range(nclips), n)
    micro, _ = oracle.fingerprint_batch(pcm.reshape(-1), np.arange(nclips + 1) * n, sr, nthreads=8, want_db=False)
    nf = n // 256
    uuids = ["%08x-3333-4000-8000-%012x" % (c * 2654435761 % 2**32, c) for c in range(nclips)]
    clip = np.repeat(np.arange(nclips), nf)
    qn = 256 * 24
    qs = [tfp_lib.synth_pcm(SEED, [c], qn, offsets=[256 * o])[0] for c, o in ((0, 0), (2, 7), (5, 36), (3, 20))]
    qs.append(tfp_lib.synth_pcm(SEED + 1, [9], qn)[0])  # enrolled nowhere
    qflat, qoff = np.concatenate(qs), np.arange(len(qs) + 1) * qn
    qmicro, qdb = oracle.fingerprint_batch(qflat, qoff, sr, nthreads=8)
    engine.index_clear()
    try:
        for c in range(nclips):
            engine.index_add(uuids[c], micro[c * nf:(c + 1) * nf, 0], micro[c * nf:(c + 1) * nf, 1])
        st = engine.fingerprint_stats()
        fr = engine.fingerprint_batch(qflat, qoff, sr)
        assert_frames_equal(fr, qmicro, qdb)
        foff = np.arange(len(qs) + 1) * (qn // 256)
        found_any = 0
        for coefs, tol in ((1, 0.45), (1, 0.001), (2, 0.1)):
            p = tfp_lib.params(coefs, tol)
            got, gfc = engine.search_pcm_batch(qflat, qoff, p, sample_rate=sr)
            want, wfc = engine.search_batch(fr, foff, p)
            assert got == want and list(gfc) == list(wfc), (coefs, tol)
            for i in range(len(qs)):
                a, b = foff[i], foff[i + 1]
                found, w, mc, fc = oracle.search(micro[:, 0], micro[:, 1], clip, uuids, qdb[a:b, 0], qdb[a:b, 1], coefs, tol,
                                                 -1, -1)
                exp = (uuids[w], mc, fc) if found else None
                g = None if got[i] is None else (got[i]["audio_uuid"], got[i]["match_count"], got[i]["frame_count"])
                assert g == exp, (i, coefs, tol)
                found_any += found
        assert found_any >= 4
        assert_only_kernel(engine, st, "generic_i16")
    finally:
        engine.index_clear()


def test_bad_sample_rate_is_refused(engine, tfp_lib):
    """The engine refuses exactly the rates build_tables refuses (<= 0: no positive rate reaches its
    ms_maxbin > 500 branch) with TFP_E_ARG and "bad sample rate", from every form that takes a rate, and
    goes on working."""
    from tiresias_amd import Live, Stream
    pcm = tfp_lib.synth_pcm(SEED, [0], 1000)[0]
    calls = [lambda: engine.fingerprint(pcm, 0),
             lambda: engine.fingerprint_batch(pcm, [0, 1000], -8000),
             lambda: engine.fingerprint_f32_batch(pcm.astype(np.float32), [0, 1000], 0),
             lambda: engine.plan([0, 1000], 0),
             lambda: Stream(engine, 1, 1000, sample_rate=0),
             lambda: Live(engine, 1, 1000, sample_rate=0)]
    for i, call in enumerate(calls):
        with pytest.raises(tfp_lib.TfpError) as ei:
            call()
        assert ei.value.code == -1, i  # TFP_E_ARG
        assert "bad sample rate" in str(ei.value), (i, str(ei.value))
    assert len(engine.fingerprint(pcm, 2**31 - 1)) == 4
