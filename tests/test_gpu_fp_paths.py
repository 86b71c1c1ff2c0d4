"""Every fingerprint launch path at its edges, with the path asserted.

The engine has four fingerprint launches (launch_fingerprint / launch_fingerprint_f32,
csrc/tfp_kernels.hip): the small 8 kHz launch (4-frame tiles), the throughput 8 kHz launch, and the
generic kernel over int16 and over fp32 samples. Which one a call takes depends on the batch, so
each test here asserts it with the launch counter (Engine.fingerprint_stats) and compares every
frame with the CPU oracle bit for bit: m1, m2, and q1 / q2 with NaN equal to NaN. No tolerances.

The inputs are the hard ones: a ragged batch whose clips start on every sample residue (odd
starts take the throughput kernel's two-word path, the clip ends its edge mask), and stream
windows after odd-sized ticks, read back frame by frame (Stream.window_frames)."""
import ctypes as C

import numpy as np
import pytest

from fp_util import assert_frames_equal, assert_only_kernel, launches_since
from test_gpu_parity import _engine_with, _sparse_cases

pytestmark = pytest.mark.gpu

SEED_DB = 0x7153A1
TFP_E_ARG = -1

LENGTHS = [0, 1, 2, 255, 256, 257, 511, 512, 513, 767, 1023, 1024, 1025, 4095, 4096, 4097, 4351, 4353, 8191, 12345]
KINDS = ["noise", "tiny", "silence", "altfull", "dc", "sparse0", "sparse1", "sparse2", "sparse3", "sparse4", "synth"]
NCLIPS = 300   # 15 rounds of LENGTHS: ~715 k samples, 2910 frames
NHEAD = 40     # the batch cut to a small one


def _clip(tfp_lib, rng, kind, n, i):
    if kind == "noise":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    if kind == "tiny":
        return rng.integers(-2, 3, n).astype(np.int16)
    if kind == "silence":
        return np.zeros(n, np.int16)
    if kind == "altfull":
        return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "dc":
        return np.full(n, -32768, np.int16)
    if kind.startswith("sparse"):  # the five _sparse_cases kinds, built at >= 512 samples and cut to n
        return _sparse_cases(nclips=5, n=max(n, 512), seed=1000 + i)[int(kind[-1])][:n]
    return tfp_lib.synth_pcm(SEED_DB, [i], n)[0] if n else np.zeros(0, np.int16)


class Ragged:
    pass


@pytest.fixture(scope="module")
def ragged(oracle, tfp_lib):
    """The ragged edge batch and its oracle frames, built once (host only)."""
    rng = np.random.default_rng(0xF9)
    lens = np.concatenate([rng.permutation(LENGTHS) for _ in range(NCLIPS // len(LENGTHS))])
    clips = [_clip(tfp_lib, rng, KINDS[i % len(KINDS)], int(n), i) for i, n in enumerate(lens)]
    assert [len(c) for c in clips] == list(lens)
    r = Ragged()
    r.clips = clips
    r.flat = np.concatenate(clips)
    r.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r.foff = np.concatenate([[0], np.cumsum((lens + 255) // 256)]).astype(np.int64)
    # the batch itself: long clips start on every sample residue mod 8 (every 16-byte phase, both
    # parities), and the shortest clips on both parities
    nfr = (lens + 255) // 256
    start = r.off[:-1]
    assert {int(s) % 8 for s, f in zip(start, nfr) if f >= 17} == set(range(8))
    assert {int(s) % 2 for s, f in zip(start, nfr) if 1 <= f <= 2} == {0, 1}
    assert {KINDS[i % len(KINDS)] for i, f in enumerate(nfr) if f >= 17} == set(KINDS)
    r.micro, r.db = oracle.fingerprint_batch(r.flat, r.off, nthreads=8)
    assert len(r.micro) == r.foff[-1] > 2500
    return r


def test_host_batch_takes_throughput_kernel(engine, ragged):
    st = engine.fingerprint_stats()
    fr = engine.fingerprint_batch(ragged.flat, ragged.off)
    assert_only_kernel(engine, st, "throughput8k", "the batch is a small one now: grow NCLIPS")
    assert_frames_equal(fr, ragged.micro, ragged.db)
    assert np.array_equal(fr["frame_idx"], np.concatenate([np.arange(n) for n in np.diff(ragged.foff)]))


@pytest.mark.parametrize("nsamples", [4100 * 256 + 77, 4097 * 256])
def test_one_long_clip_takes_throughput_kernel(engine, oracle, tfp_lib, nsamples):
    """One clip of more than 4096 frames (a long recording through tfp_fingerprint_pcm): the throughput
    launch without the layout loads. Its first and last tiles read the clip through the buffer
    resource, as any clip's do."""
    pcm = tfp_lib.synth_pcm(0x10C6, [3], nsamples)[0]
    st = engine.fingerprint_stats()
    fr = engine.fingerprint(pcm)
    assert_only_kernel(engine, st, "throughput8k", "the clip is a small batch now: lengthen it")
    _, db, micro = oracle.fingerprint(pcm)
    assert_frames_equal(fr, micro, db)


def test_host_batch_head_takes_small_kernel(engine, ragged):
    st = engine.fingerprint_stats()
    fr = engine.fingerprint_batch(ragged.flat[:ragged.off[NHEAD]], ragged.off[:NHEAD + 1])
    assert_only_kernel(engine, st, "small8k", "the head is no small batch now: shrink NHEAD")
    nf = ragged.foff[NHEAD]
    assert_frames_equal(fr, ragged.micro[:nf], ragged.db[:nf])


@pytest.mark.parametrize("knob,kernel", [(("TFP_GENERIC", "1"), "generic_i16"),
                                         (("TFP_RARE_THR_LOG2", "100"), "throughput8k")])
def test_host_batch_kernel_variants(ragged, tfp_lib, knob, kernel):
    """The generic int16 kernel at 8 kHz, and the throughput kernel with every non-zero bin on the
    real split's spec-order slow path."""
    eng = _engine_with(tfp_lib, {knob[0]: knob[1]})  # knobs are read once, at engine creation
    try:
        st = eng.fingerprint_stats()
        fr = eng.fingerprint_batch(ragged.flat, ragged.off)
        assert_only_kernel(eng, st, kernel)
    finally:
        eng.close()
    assert_frames_equal(fr, ragged.micro, ragged.db)


def test_f32_batch_takes_generic_f32_kernel(engine, oracle, ragged):
    """The same samples as fp32 values (int16 / 32768, exact) against the oracle's fp32 form."""
    x = ragged.flat.astype(np.float32) / np.float32(32768)
    st = engine.fingerprint_stats()
    fr = engine.fingerprint_f32_batch(x, ragged.off)
    assert_only_kernel(engine, st, "generic_f32")
    want = [oracle.fingerprint_f32(x[a:b]) for a, b in zip(ragged.off[:-1], ragged.off[1:])]
    assert_frames_equal(fr, np.concatenate([w[2] for w in want]), np.concatenate([w[1] for w in want]))


@pytest.mark.parametrize("shift", [0, 1])
def test_device_plan_takes_throughput_kernel(engine, ragged, shift):
    """tfp_fingerprint_device states no alignment for d_pcm: shift = 1 puts the batch one sample
    into the buffer, so the base is only 2-byte aligned and every clip's parity flips."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = len(ragged.flat)
    buf = torch.zeros(n + 64, dtype=torch.int16, device="cuda")
    buf[shift:shift + n] = torch.from_numpy(ragged.flat).cuda()
    plan = engine.plan(ragged.off)
    assert plan.nframes == ragged.foff[-1]
    micro = torch.zeros((plan.nframes, 2), dtype=torch.int32, device="cuda")
    db = torch.zeros((plan.nframes, 2), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    st = engine.fingerprint_stats()
    engine.fingerprint_device(plan, buf.data_ptr() + 2 * shift, micro.data_ptr(), db.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_only_kernel(engine, st, "throughput8k")
    assert buf.data_ptr() % 16 == 0
    m, q = micro.cpu().numpy(), db.cpu().numpy()
    fr = np.zeros(plan.nframes, [("m1", "<i4"), ("m2", "<i4"), ("q1", "<f8"), ("q2", "<f8")])
    fr["m1"], fr["m2"], fr["q1"], fr["q2"] = m[:, 0], m[:, 1], q[:, 0], q[:, 1]
    assert_frames_equal(fr, ragged.micro, ragged.db)


def test_single_clips_at_odd_host_address_take_small_kernel(engine, ragged):
    """One clip of each length at a time, from a host address that is only 2-byte aligned."""
    seen = {}
    for c, n in enumerate(np.diff(ragged.off)):
        seen.setdefault(int(n), c)
    assert sorted(seen) == sorted(LENGTHS)
    st = engine.fingerprint_stats()
    for n, c in sorted(seen.items()):
        big = np.zeros(n + 2, np.int16)
        k = 1 if big.ctypes.data % 4 == 0 else 2  # the sample of `big` at an address = 2 mod 4
        odd = big[k:k + n]
        odd[:] = ragged.clips[c]
        assert (big.ctypes.data + 2 * k) % 4 == 2 and odd.flags["C_CONTIGUOUS"]
        assert n == 0 or odd.ctypes.data == big.ctypes.data + 2 * k
        fr = engine.fingerprint(odd)
        a, b = ragged.foff[c], ragged.foff[c + 1]
        assert_frames_equal(fr, ragged.micro[a:b], ragged.db[a:b])
    assert_only_kernel(engine, st, "small8k")


# ------------------------------------------------------------------------------- stream seams

class Enrolled:
    pass


@pytest.fixture(scope="module")
def enrolled(oracle, tfp_lib):
    """8 synthetic clips and their oracle rows (host only); each test enrols them itself."""
    e = Enrolled()
    e.nclips, e.n = 8, 8000 * 4
    e.pcm = tfp_lib.synth_pcm(SEED_DB, range(e.nclips), e.n)
    e.micro, _ = oracle.fingerprint_batch(e.pcm.reshape(-1), np.arange(e.nclips + 1) * e.n, nthreads=8, want_db=False)
    e.nf = (e.n + 255) // 256
    e.uuids = ["%08x-2222-4000-8000-%012x" % (c * 2654435761 % 2**32, c) for c in range(e.nclips)]
    e.clip = np.repeat(np.arange(e.nclips), e.nf)
    return e


def _enrol(engine, e):
    engine.index_clear()
    for c in range(e.nclips):
        engine.index_add(e.uuids[c], e.micro[c * e.nf:(c + 1) * e.nf, 0], e.micro[c * e.nf:(c + 1) * e.nf, 1])


TICKS = [1, 159, 160, 161, 7, 255, 257, 1000, None]  # 1000: min(W, 1000); None: W
NPUSH = 40


@pytest.mark.parametrize("W", [255, 256, 257, 513, 4001, 4096])
def test_stream_window_frames_at_seams(engine, oracle, tfp_lib, enrolled, W):
    """Ticks of odd and even sizes, ticks that wrap the ring and ticks of a whole window: after every
    push each full channel's window, read back frame by frame, equals the oracle's fingerprint of
    that channel's last W samples, and on every third push the search result the oracle's."""
    from tiresias_amd import Stream
    e = enrolled
    _enrol(engine, e)
    nch = 3
    seq = [T for T in (min(W, 1000) if t == 1000 else W if t is None else t for t in TICKS) if T <= W]
    ticks = [seq[i % len(seq)] for i in range(NPUSH)]
    total = sum(ticks)
    rng = np.random.default_rng(W)
    src = np.stack([
        np.resize(tfp_lib.synth_pcm(SEED_DB, [5], e.n - 1000, offsets=[1000])[0], total),  # an enrolled clip, looped
        rng.integers(-32768, 32768, total).astype(np.int16),
        np.where(np.arange(total) % 2 == 0, 32767, -32768).astype(np.int16)])
    ps = [(1, 0.45), (2, 0.001)]
    st = Stream(engine, nch, W)
    F = (W + 255) // 256
    stats0 = engine.fingerprint_stats()
    hist = [np.zeros(0, np.int16) for _ in range(nch)]
    pos = wpos = 0
    checked = odd_checked = wrap_checked = searched = found_any = 0
    try:
        for i, T in enumerate(ticks):
            if i == NPUSH // 2:
                st.reset(1)
                hist[1] = np.zeros(0, np.int16)
                assert len(st.window_frames(1)) == 0
            blk = src[:, pos:pos + T]
            pos += T
            wrapped = wpos + T > W   # the tick's samples cross the ring's end
            wpos = (wpos + T) % W    # where every window starts after this push
            hist = [np.concatenate([h, b])[-W:] for h, b in zip(hist, blk)]
            coefs, tol = ps[(i // 3) % 2]
            res = st.push(blk, tfp_lib.params(coefs, tol) if i % 3 == 2 else None)
            for c in range(nch):
                fr = st.window_frames(c)
                if len(hist[c]) < W:
                    assert len(fr) == 0, (i, c)
                    assert res is None or res[c] is None
                    continue
                _, qdb, micro = oracle.fingerprint(hist[c])
                assert len(fr) == F
                assert_frames_equal(fr, micro, qdb)
                assert np.array_equal(fr["frame_idx"], np.arange(F))
                checked += 1
                odd_checked += wpos % 2
                wrap_checked += wrapped
                if res is None:
                    continue
                found, w, mc, fc = oracle.search(e.micro[:, 0], e.micro[:, 1], e.clip, e.uuids, qdb[:, 0], qdb[:, 1],
                                                 coefs, tol, -1, -1)
                exp = (e.uuids[w], mc, fc) if found else None
                got = None if res[c] is None else (res[c]["audio_uuid"], res[c]["match_count"], res[c]["frame_count"])
                assert got == exp, (i, c, coefs, tol)
                searched += 1
                found_any += found
        d = launches_since(engine, stats0)
    finally:
        st.close()
        engine.index_clear()
    assert d["throughput8k"] >= checked // nch and d["small8k"] == d["generic_i16"] == d["generic_f32"] == 0, d
    assert checked > NPUSH and odd_checked > 0 and wrap_checked > 0 and searched >= 2 * nch, \
        (checked, odd_checked, wrap_checked, searched)
    if W >= 4001:
        assert found_any > 0  # (windows of a few frames may match nothing; 16-frame windows of an enrolled clip do)


def test_stream_read_out_leaves_the_stream_alone(engine, oracle, tfp_lib, enrolled):
    """Two streams fed the same ticks, one read out after every push: same results, same frames."""
    from tiresias_amd import Stream
    _enrol(engine, enrolled)
    W, nch = 513, 2
    rng = np.random.default_rng(5)
    a, b = Stream(engine, nch, W), Stream(engine, nch, W)
    p = tfp_lib.params(2, 0.001)
    try:
        for T in [161, 255, 97, 513, 1, 160, 257]:
            blk = rng.integers(-32768, 32768, (nch, T)).astype(np.int16)
            ra = a.push(blk, p)
            for c in range(nch):
                a.window_frames(c)
                a.window_frames(c)
            assert b.push(blk, p) == ra
        for c in range(nch):
            fa, fb = a.window_frames(c), b.window_frames(c)
            assert len(fa) == 3 and fa.tobytes() == fb.tobytes()
    finally:
        a.close()
        b.close()
        engine.index_clear()


def test_stream_argument_checks(engine, tfp_lib):
    """Bad tick sizes, channels and capacities are TFP_E_ARG, and the stream and engine go on working."""
    from tiresias_amd import Stream, lib
    W, nch = 600, 2
    st = Stream(engine, nch, W)
    try:
        def arg_error(call):
            with pytest.raises(tfp_lib.TfpError) as ei:
                call()
            assert ei.value.code == TFP_E_ARG

        arg_error(lambda: st.push(np.zeros((nch, W + 1), np.int16)))   # T > W
        arg_error(lambda: st.push(np.zeros((nch, 0), np.int16)))       # T == 0
        one = np.zeros((nch, 1), np.int16)
        assert lib().tfp_stream_push(st._h, one.ctypes.data, -1, None, None) == TFP_E_ARG  # T < 0
        arg_error(lambda: st.reset(nch))
        arg_error(lambda: st.window_frames(nch))
        arg_error(lambda: st.window_frames(-1))
        pcm = np.random.default_rng(9).integers(-32768, 32768, (nch, W)).astype(np.int16)
        assert st.push(pcm) is None
        F = (W + 255) // 256
        out = np.zeros(F, tfp_lib.FRAME_DTYPE)
        got = C.c_int64(-1)
        assert lib().tfp_stream_window_frames(st._h, 0, out.ctypes.data, F - 1, C.byref(got)) == TFP_E_ARG
        assert got.value == F and not out.view(np.uint8).any()
        assert lib().tfp_stream_window_frames(st._h, 0, out.ctypes.data, F, None) == TFP_E_ARG
        # everything still works
        fr = st.window_frames(1)
        assert len(fr) == F
        assert fr.tobytes() == engine.fingerprint(pcm[1]).tobytes()
    finally:
        st.close()
