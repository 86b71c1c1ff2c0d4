"""Stream ordering of the device forms (tfp_fingerprint_device, tfp_index_add_device, tfp_search_device,
tfp_search_q_device, tfp_synth_pcm_device), with a producer still pending on the caller's stream when the
form is called and a consumer queued behind it with no host wait in between.

Every case runs on a stream P, the caller's: the HIP null stream (torch's default stream) with
stream = NULL, where the engine works on its own non-blocking stream between two event edges
(NullStreamOrder, csrc/tfp_engine.cpp), or a torch side stream whose handle is passed.

1. The form's device input holds a decoy: valid data of the same shape whose oracle result differs
   from the real one at every clip / query compared. Every output buffer holds 0x5A5A5A5A words.
2. A chain of in-place elementwise torch ops on a large scratch tensor keeps P busy (the delay).
3. Behind it on P: the real input is copied over the decoy, device to device, and `ready` is recorded.
4. The form is called, with the producer of its input still pending.
5. At once, with no host wait, every output is cloned on P.
6. After a synchronise the clones equal the CPU oracle's result of the real input.

A form that read its input ahead of P's earlier work computes the decoy's result; a form whose output
edge is missing leaves the sentinel (or a part of it) in the clone. The window is asserted in every
case: for tfp_fingerprint_device, which returns without waiting, `ready` has not happened right after
the call and right after the clones are queued; for the other four, which wait for their stream,
`ready` has not happened right before the call and the call lasts at least half the calibrated delay.
A case whose window was closed fails with "window closed"; it is run again, at most twice with the
delay doubled, only for that reason: a wrong result fails at once.

A plan's layout is 16-frame tiles whatever the batch size, so tfp_fingerprint_device runs the
throughput 8 kHz kernel on both batches here (the 4-frame-tile kernel belongs to the host forms): the
64-clip batch is its 256-tile launch of one partial wave of blocks, the batch of
tests/test_gpu_fused_finish.py its ragged one. With d_db a second kernel (finish_db_kernel) follows on
the same stream; without, the tile tail finishes in the one launch.

The searches run over an index of made-up rows at 16 and 17 dB and noise queries whose loud and soft
shares decide winner and count (see _rows, _level_queries): synthetic clips' own rows almost never lie
within a small tolerance of an integer, which is all the reference's search matches.

tfp_synth_pcm_device has no input, so its in-edge is a write-after-write one: the sentinel fill of
d_out is queued on P behind the delay, and samples written before it would be overwritten."""
import math
import time

import numpy as np
import pytest

from fp_util import assert_only_kernel
from test_gpu_fused_finish import LENGTHS, ROUNDS

pytestmark = pytest.mark.gpu

SEED = 0x7153A1
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A
NCLIPS, CLIP_N = 64, 16000  # 2 s at 8 kHz: 63 frames a clip
NQ, QUERY_N = 32, 8000      # 1 s: 32 frames a query
CLIP_F, QUERY_F = (CLIP_N + 255) // 256, (QUERY_N + 255) // 256
STREAMS = ("default", "side")
# (coefs, tolerance) per search form: coefs 1 takes the vote path, coefs 2 the general path
PCM_PARAMS = ((1, 0.05), (2, 0.45))
Q_PARAMS = ((1, 0.001), (2, 0.5))
# The delay: at least this long, at least 200 x the host's enqueue path of the asynchronous form (the
# call and the clones of its outputs, measured unloaded) and at least 20 x the slowest waiting form's
# unloaded call-to-completion time, so that "the call lasted half the delay" cannot be the form's own
# work. On the MI355X the enqueue path takes 0.10 to 0.17 ms and the slowest form 0.10 ms at these shapes
# (profiles/r08/stream_order_calibration.txt), so the floor decides there: 40 ms, 240 x the enqueue path
# at the least, and short enough that the 21 cases take about two seconds together. A slower host
# lengthens the delay by the first rule.
MIN_DELAY_MS = 40.0
SCRATCH_ELEMS = 1 << 26  # fp32 per row: one in-place op moves 512 MiB, far longer than its launch takes


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Bag:
    pass


def _per_clip_differ(a, b, foff):
    return all(not np.array_equal(a[foff[c]:foff[c + 1]], b[foff[c]:foff[c + 1]]) for c in range(len(foff) - 1))


def _pcm_batch(oracle, real, decoy, off, want_db=True):
    """A fingerprint batch: real and decoy PCM of one layout, the oracle's frames of both, every clip's differing."""
    b = Bag()
    b.real, b.decoy, b.off = real, decoy, np.ascontiguousarray(off, np.int64)
    b.micro, b.db = oracle.fingerprint_batch(real, b.off, nthreads=8, want_db=want_db)
    b.decoy_micro, b.decoy_db = oracle.fingerprint_batch(decoy, b.off, nthreads=8, want_db=want_db)
    nfr = (np.diff(b.off) + 255) // 256
    b.foff = np.concatenate([[0], np.cumsum(nfr)]).astype(np.int64)
    b.nframes = int(b.foff[-1])
    assert _per_clip_differ(b.micro, b.decoy_micro, b.foff), "a decoy clip has the real clip's micro-units"
    if want_db:
        assert _per_clip_differ(b.db.view(np.uint64), b.decoy_db.view(np.uint64), b.foff)
    return b


def _tiles_batch(oracle, tfp_lib):
    """The just-over-256-tile batch of test_gpu_fused_finish.py, and a decoy of full-range noise in its layout."""
    rng = np.random.default_rng(0xF1)
    lens = np.array(LENGTHS * ROUNDS, np.int64)
    clips = []
    for i, n in enumerate(lens):
        kind = i % 4
        if kind == 0:
            c = rng.integers(-32768, 32768, n).astype(np.int16)
        elif kind == 1:
            c = tfp_lib.synth_pcm(SEED, [i], int(n))[0]
        elif kind == 2:
            c = rng.integers(-3, 4, n).astype(np.int16)
        else:
            c = np.zeros(n, np.int16)
        clips.append(c)
    real = np.concatenate(clips)
    # never a zero sample, the opposite sign of a real non-zero one: a 1-sample clip differs too
    mag = np.random.default_rng(0xDEC0).integers(9000, 32768, len(real)).astype(np.int16)
    decoy = np.where(real > 0, -mag, mag).astype(np.int16)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert 256 < int((((lens + 255) // 256 + 15) // 16).sum()) <= 300
    return _pcm_batch(oracle, real, decoy, off, want_db=False)


def _rows(seed, swap):
    """The index's rows, clip c's 63 all at max1 = 16 (+ swap + c even) or 17 dB within a micro-unit of noise
    below the tightest tolerance, max2 about 17.05 dB (the reference matches a row whose max1 lies within the
    tolerance of the query frame's max1 cut to an integer, fp_handler.c:290, so only such rows ever match)."""
    rng = np.random.default_rng(seed)
    k = 16 + (np.arange(NCLIPS) + swap) % 2
    m1 = np.repeat(k, CLIP_F) * 1000000 + rng.integers(-900, 901, NCLIPS * CLIP_F)
    m2 = 17050000 + rng.integers(-50000, 50001, NCLIPS * CLIP_F)
    return np.stack([m1, m2], 1).astype(np.int32)


def _level_queries(seed, loud_hops):
    """Noise queries of a second, query i's first loud_hops[i] hops loud (max1 in [16, 17) dB) and the rest
    soft ([17, 18)): the loud frames match the clips at 16 dB, the soft ones those at 17 dB, and the larger
    share decides the winner and its count."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((NQ, QUERY_N))
    x /= np.abs(x).max()
    amp = np.full((NQ, QUERY_N), 64.0)
    for i, h in enumerate(loud_hops):
        amp[i, :256 * h] = 8192.0
    return np.round(x * amp).astype(np.int16).reshape(-1)


def _build_data(oracle, tfp_lib):
    d = Bag()
    off = np.arange(NCLIPS + 1, dtype=np.int64) * CLIP_N
    d.enrol = _pcm_batch(oracle, tfp_lib.synth_pcm(SEED, range(NCLIPS), CLIP_N).reshape(-1),
                         tfp_lib.synth_pcm(SEED, range(1000, 1000 + NCLIPS), CLIP_N).reshape(-1), off)
    assert d.enrol.nframes == NCLIPS * CLIP_F and CLIP_F == 63
    d.tiles = _tiles_batch(oracle, tfp_lib)
    d.uuids = ["%08x-0000-4000-8000-%012x" % (i * 7919 % 65536, i) for i in range(NCLIPS)]
    d.rows_off = np.arange(NCLIPS + 1, dtype=np.int64) * CLIP_F
    d.rows, d.decoy_rows = _rows(0x1D, 0), _rows(0x2D, 1)
    assert _per_clip_differ(d.rows, d.decoy_rows, d.rows_off)
    d.queries = _pcm_batch(oracle, _level_queries(0xA1, [20 + i % 10 for i in range(NQ)]),
                           _level_queries(0xA2, [3 + i % 10 for i in range(NQ)]),
                           np.arange(NQ + 1, dtype=np.int64) * QUERY_N)
    assert d.queries.nframes == NQ * QUERY_F
    row_clip = np.repeat(np.arange(NCLIPS, dtype=np.int32), CLIP_F)

    def winners(rows, db, coefs, tol):
        out = []
        for i in range(NQ):
            q = db[i * QUERY_F:(i + 1) * QUERY_F]
            found, w, mc, _ = oracle.search(rows[:, 0], rows[:, 1], row_clip, d.uuids, q[:, 0], q[:, 1], coefs, tol)
            out.append((w, mc) if found else None)
        return out

    def differ(a, b, *what):  # a stale read cannot pass: every query's result differs, and the real one is a match
        for i in range(NQ):
            assert a[i] is not None and a[i] != b[i], (what, i, a[i], b[i])

    d.want, d.decoy_want = {}, {}
    for coefs, tol in sorted(set(PCM_PARAMS + Q_PARAMS)):
        d.want[coefs, tol] = winners(d.rows, d.queries.db, coefs, tol)
        d.decoy_want[coefs, tol] = winners(d.rows, d.queries.decoy_db, coefs, tol)
        differ(d.want[coefs, tol], d.decoy_want[coefs, tol], coefs, tol)
        assert len(set(d.want[coefs, tol])) >= 8  # (counts from 20 to 29 frames)
    # tfp_index_add_device's stale read: the real queries over the decoy rows
    differ(d.want[1, 0.001], winners(d.decoy_rows, d.queries.db, 1, 0.001), "decoy rows")
    return d


@pytest.fixture(scope="module")
def data(oracle, tfp_lib):
    """Inputs, decoys and the oracle's results of both (CPU only, computed once)."""
    return _build_data(oracle, tfp_lib)


def _stream(torch, which):
    """(P, the handle the form is given)."""
    if which == "default":
        P = torch.cuda.default_stream()
        assert P.cuda_stream == 0  # the HIP null stream: the form's stream == NULL branch
        return P, 0
    P = torch.cuda.Stream()
    assert P.cuda_stream != 0
    return P, P.cuda_stream


def _queue_delay(torch, P, row, nops):
    with torch.cuda.stream(P):
        for _ in range(nops):
            row.mul_(-1.0)


def _pending(torch, cal, P, scale, copies, row=0):
    """Steps 2 and 3 on P: the delay, the copies (dst, src) over the decoys, the event behind them."""
    _queue_delay(torch, P, cal.scratch[row], cal.nops * scale)
    with torch.cuda.stream(P):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(P)
    return ready


def _run(case):
    """case(scale) -> "" or why its window was closed; raises at once on a wrong result."""
    why = ""
    for attempt in range(3):
        why = case(1 << attempt)
        if not why:
            return
        print("window closed at delay x%d: %s" % (1 << attempt, why))
    pytest.fail("window closed: " + why)


def _async_window(open_after_call, open_after_clones):
    if open_after_call and open_after_clones:
        return ""
    return "the producer had finished %s" % ("when the call returned" if not open_after_call else "when the clones were queued")


def _waited(cal, scale, pending_before, host_ms):
    if not pending_before:
        return "the producer had finished before the call"
    if host_ms < 0.5 * cal.delay_ms * scale:
        return "the call took %.2f ms of a %.1f ms delay" % (host_ms, cal.delay_ms * scale)
    return ""


def _timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def _sentinel(torch, shape, dtype):
    if dtype == torch.float64:
        return torch.full(shape, SENT64, dtype=torch.int64, device="cuda").view(torch.float64)
    return torch.full(shape, SENT64 if dtype == torch.int64 else SENT32, dtype=dtype, device="cuda")


def _assert_micro(got, b, what=""):
    g = got.cpu().numpy()
    if not np.array_equal(g, b.micro):
        bad = (g != b.micro).any(axis=1)
        pytest.fail("%s micro-units: %d of %d frames wrong, %d of them the sentinel, %d the decoy's" % (
            what, bad.sum(), len(bad), (g[bad] == SENT32).all(axis=1).sum(), (g[bad] == b.decoy_micro[bad]).all(axis=1).sum()))


def _assert_db(got, b, what=""):
    g = got.cpu().numpy()
    same = (g.view(np.uint64) == b.db.view(np.uint64)) | (np.isnan(g) & np.isnan(b.db))  # (fp_util: a NaN is a NaN)
    if not same.all():
        bad = ~same.all(axis=1)
        pytest.fail("%s frame values: %d of %d frames wrong, %d of them the sentinel, %d the decoy's" % (
            what, bad.sum(), len(bad), (g.view(np.uint64)[bad] == SENT64).all(axis=1).sum(),
            (g.view(np.uint64)[bad] == b.decoy_db.view(np.uint64)[bad]).all(axis=1).sum()))


def _enrol(rig):
    """The real rows as the index; key_of: a clip's tie-break key (its uuid's rank)."""
    eng, d = rig.engine, rig.data
    eng.index_clear()
    eng.index_add_batch(d.uuids, d.rows_off, d.rows[:, 0], d.rows[:, 1])
    eng.index_commit()
    rig.key_of = {eng.uuid_of_key(k): k for k in range(NCLIPS)}
    assert sorted(rig.key_of) == sorted(d.uuids)


def _want_keys(rig, coefs, tol, decoy=False):
    want = (rig.data.decoy_want if decoy else rig.data.want)[coefs, tol]
    return np.array([0 if r is None else (r[1] << 32) | rig.key_of[rig.data.uuids[r[0]]] for r in want], np.uint64)


def _assert_keys(rig, got, coefs, tol):
    g = got.cpu().numpy().view(np.uint64)
    want = _want_keys(rig, coefs, tol)
    if not np.array_equal(g, want):
        bad = g != want
        pytest.fail("keys (coefs %d, tolerance %g): %d of %d queries wrong, %d of them the sentinel, %d the decoy's" % (
            coefs, tol, bad.sum(), NQ, (g[bad] == SENT64).sum(), (g[bad] == _want_keys(rig, coefs, tol, True)[bad]).sum()))


def _query_frames(db):
    from tiresias_amd.engine import FRAME_DTYPE
    fr = np.zeros(len(db), FRAME_DTYPE)
    fr["q1"], fr["q2"] = db[:, 0], db[:, 1]
    return fr


def _assert_host_results(rig, res, coefs, tol):
    got = [None if r is None else (r["audio_uuid"], r["match_count"]) for r in res]
    assert got == [None if r is None else (rig.data.uuids[r[0]], r[1]) for r in rig.data.want[coefs, tol]]


def _search_call(rig, form, coefs, tol, handle):
    """(real input, decoy input, call(buffer, keys)) of one search form on the query batch."""
    torch, eng, q = rig.torch, rig.engine, rig.data.queries
    p = rig.tfp_lib.params(coefs, tol)
    if form == "pcm":
        plan = eng.plan(q.off)
        assert plan.nframes == q.nframes
        return (torch.from_numpy(q.real).cuda(), torch.from_numpy(q.decoy).cuda(),
                lambda buf, keys: eng.search_device(plan, buf.data_ptr(), p, keys.data_ptr(), handle))
    return (torch.from_numpy(q.db).cuda(), torch.from_numpy(q.decoy_db).cuda(),
            lambda buf, keys: eng.search_q_device(buf.data_ptr(), q.foff, p, keys.data_ptr(), handle))


@pytest.fixture(scope="module")
def rig(torch_cuda, engine, tfp_lib, data):
    """The warm-up (first uses of tables, of the log table and of the index wait on the engine's stream, which
    would close a window), then the delay's calibration: one chain op's time, every form's unloaded time."""
    torch = torch_cuda
    r = Bag()
    r.torch, r.engine, r.tfp_lib, r.data = torch, engine, tfp_lib, data
    cal = r.cal = Bag()
    cal.scratch = torch.ones((2, SCRATCH_ELEMS), dtype=torch.float32, device="cuda")
    D = torch.cuda.default_stream()
    _queue_delay(torch, D, cal.scratch[0], 10)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(D)
    cal.op_host_ms = _timed(lambda: _queue_delay(torch, D, cal.scratch[0], 50)) / 50
    t1.record(D)
    torch.cuda.synchronize()
    cal.op_ms = t0.elapsed_time(t1) / 50
    assert cal.op_ms > 3 * cal.op_host_ms, "a chain op is queued no faster than it runs: no delay builds up"

    unloaded = cal.unloaded = {}

    def completes(name, f, times=2):  # the first call warms up, the last is timed to its completion
        for _ in range(times):
            torch.cuda.synchronize()
            unloaded[name] = _timed(lambda: (f(), torch.cuda.synchronize()))

    side = torch.cuda.Stream()
    enqueue = []
    for b, name in ((data.enrol, "fingerprint"), (data.tiles, "fingerprint_tiles")):
        pcm = torch.from_numpy(b.real).cuda()
        plan = engine.plan(b.off)
        micro = _sentinel(torch, (b.nframes, 2), torch.int32)
        db = _sentinel(torch, (b.nframes, 2), torch.float64)
        for handle in (0, side.cuda_stream):
            completes(name + "_db", lambda: engine.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), db.data_ptr(), handle))
            completes(name, lambda: engine.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), 0, handle))
        torch.cuda.synchronize()
        enqueue.append(_timed(lambda: (engine.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), db.data_ptr(), 0),
                                       micro.clone(), db.clone())))
        torch.cuda.synchronize()
    cal.enqueue_ms = max(enqueue)
    d_micro = torch.from_numpy(data.rows).cuda()
    for handle in (0, side.cuda_stream):
        def add():
            engine.index_clear()
            engine.index_add_device(data.uuids, data.rows_off, d_micro.data_ptr(), handle)
        completes("index_add", add)
    _enrol(r)
    for form, params in (("pcm", PCM_PARAMS), ("q", Q_PARAMS)):
        for coefs, tol in params:
            for handle in (0, side.cuda_stream):
                real, _, call = _search_call(r, form, coefs, tol, handle)
                keys = _sentinel(torch, (NQ,), torch.int64)
                completes("search_%s_c%d" % (form, coefs), lambda: call(real, keys))
                _assert_keys(r, keys, coefs, tol)
    engine.search_batch(_query_frames(data.queries.db), data.queries.foff, tfp_lib.params(1, 0.001))
    out = torch.empty((6, 5000), dtype=torch.int16, device="cuda")
    for handle in (0, side.cuda_stream):
        completes("synth", lambda: engine.synth_device(SEED, range(6), 5000, out.data_ptr(), stream=handle))
    engine.index_clear()

    slowest_wait = max(v for k, v in unloaded.items() if not k.startswith("fingerprint"))
    cal.delay_ms = max(MIN_DELAY_MS, 200 * cal.enqueue_ms, 20 * slowest_wait)
    cal.nops = int(math.ceil(cal.delay_ms / cal.op_ms))
    print("\nstream-order calibration: chain op %.1f us on the GPU, %.1f us to queue; chain length %d; delay %.1f ms"
          % (cal.op_ms * 1e3, cal.op_host_ms * 1e3, cal.nops, cal.nops * cal.op_ms))
    print("stream-order calibration: asynchronous form's enqueue path (call + clones) %.3f ms" % cal.enqueue_ms)
    for k in sorted(unloaded):
        print("stream-order calibration: unloaded %s %.3f ms" % (k, unloaded[k]))
    yield r
    engine.index_clear()
    del cal.scratch
    torch.cuda.empty_cache()


# ---- tfp_fingerprint_device: returns without waiting ----------------------------------------------

def _fingerprint_case(rig, which, b, with_db, kernel=None):
    torch, eng, cal = rig.torch, rig.engine, rig.cal
    P, handle = _stream(torch, which)
    real, decoy = torch.from_numpy(b.real).cuda(), torch.from_numpy(b.decoy).cuda()
    plan = eng.plan(b.off)
    assert plan.nframes == b.nframes

    def case(scale):
        pcm = decoy.clone()
        micro = _sentinel(torch, (b.nframes, 2), torch.int32)
        db = _sentinel(torch, (b.nframes, 2), torch.float64) if with_db else None
        torch.cuda.synchronize()
        st = eng.fingerprint_stats()
        ready = _pending(torch, cal, P, scale, [(pcm, real)])
        eng.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), db.data_ptr() if with_db else 0, handle)
        open_after_call = not ready.query()
        with torch.cuda.stream(P):
            got_micro = micro.clone()
            got_db = db.clone() if with_db else None
        open_after_clones = not ready.query()
        torch.cuda.synchronize()
        if kernel:
            assert_only_kernel(eng, st, kernel)
        _assert_micro(got_micro, b)
        if with_db:
            _assert_db(got_db, b)
        return _async_window(open_after_call, open_after_clones)

    _run(case)


@pytest.mark.parametrize("which", STREAMS)
def test_fingerprint_device_with_db(rig, which):
    """Kernel + finish_db_kernel: d_micro and d_db bit-equal to the oracle's."""
    _fingerprint_case(rig, which, rig.data.enrol, True, "throughput8k")


@pytest.mark.parametrize("batch", ("enrol", "tiles"))
@pytest.mark.parametrize("which", STREAMS)
def test_fingerprint_device_fused_finish(rig, which, batch):
    """d_db = NULL, one launch: the 64-clip batch and the just-over-256-tile one."""
    _fingerprint_case(rig, which, getattr(rig.data, batch), False, "throughput8k")


# ---- the four forms that wait for their stream before they return ----------------------------------

def _waiting_call(rig, P, scale, copies, call):
    """Steps 2 to 4 for a form that waits: -> why the window was closed ("" when it was open)."""
    ready = _pending(rig.torch, rig.cal, P, scale, copies)
    pending_before = not ready.query()
    host_ms = _timed(call)
    return _waited(rig.cal, scale, pending_before, host_ms)


@pytest.mark.parametrize("which", STREAMS)
def test_index_add_device(rig, which):
    """In-edge d_micro; the stored rows read back and a search over them are the real clips'."""
    torch, eng, d = rig.torch, rig.engine, rig.data
    P, handle = _stream(torch, which)
    real, decoy = torch.from_numpy(d.rows).cuda(), torch.from_numpy(d.decoy_rows).cuda()
    foff = d.rows_off

    def case(scale):
        eng.index_clear()
        d_micro = decoy.clone()
        torch.cuda.synchronize()
        why = _waiting_call(rig, P, scale, [(d_micro, real)],
                            lambda: eng.index_add_device(d.uuids, foff, d_micro.data_ptr(), handle))
        stale = wrong = 0
        for c in range(NCLIPS):
            m1, m2 = eng.index_rows(d.uuids[c])
            rows = np.stack([m1, m2], 1)
            wrong += not np.array_equal(rows, d.rows[foff[c]:foff[c + 1]])
            stale += np.array_equal(rows, d.decoy_rows[foff[c]:foff[c + 1]])
        assert wrong == 0, "%d of %d clips' stored rows wrong, %d of them the decoy's" % (wrong, NCLIPS, stale)
        res, _ = eng.search_batch(_query_frames(d.queries.db), d.queries.foff, rig.tfp_lib.params(1, 0.001))
        _assert_host_results(rig, res, 1, 0.001)
        torch.cuda.synchronize()
        return why

    try:
        _run(case)
    finally:
        eng.index_clear()


def _search_case(rig, which, form, coefs, tol):
    torch, eng = rig.torch, rig.engine
    P, handle = _stream(torch, which)
    _enrol(rig)
    real, decoy, call = _search_call(rig, form, coefs, tol, handle)
    warm = _sentinel(torch, (NQ,), torch.int64)
    call(decoy, warm)  # this index, parameter set and stream once: the tolerance's caches are built
    torch.cuda.synchronize()

    def case(scale):
        buf = decoy.clone()
        keys = _sentinel(torch, (NQ,), torch.int64)
        torch.cuda.synchronize()
        st = eng.search_path_stats()
        why = _waiting_call(rig, P, scale, [(buf, real)], lambda: call(buf, keys))
        with torch.cuda.stream(P):
            got = keys.clone()
        torch.cuda.synchronize()
        now = eng.search_path_stats()
        took = {k: now[k] - st[k] for k in now}
        vote = took["vote_class"] + took["vote_gemm"]
        assert (vote, took["general"], took["small"], took["vote_redone"]) == ((1, 0, 0, 0) if coefs == 1 else (0, 1, 0, 0)), took
        _assert_keys(rig, got, coefs, tol)
        return why

    try:
        _run(case)
    finally:
        eng.index_clear()


@pytest.mark.parametrize("coefs,tol", PCM_PARAMS)
@pytest.mark.parametrize("which", STREAMS)
def test_search_device(rig, which, coefs, tol):
    """In-edge d_pcm (fingerprint + search on the one stream), out-edge d_keys."""
    _search_case(rig, which, "pcm", coefs, tol)


@pytest.mark.parametrize("coefs,tol", Q_PARAMS)
@pytest.mark.parametrize("which", STREAMS)
def test_search_q_device(rig, which, coefs, tol):
    """In-edge d_q, out-edge d_keys."""
    _search_case(rig, which, "q", coefs, tol)


@pytest.mark.parametrize("which", STREAMS)
def test_synth_pcm_device(rig, which):
    """No input: the sentinel fill of d_out is what the form is ordered behind; d_out == tfp_synth_pcm's."""
    torch, eng, cal = rig.torch, rig.engine, rig.cal
    P, handle = _stream(torch, which)
    clips, offsets, n = range(100, 106), [0, 256, 512, 0, 7, 99999], 5000
    host = rig.tfp_lib.synth_pcm(SEED, clips, n, offsets=offsets)

    def case(scale):
        out = torch.zeros((len(clips), n), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        _queue_delay(torch, P, cal.scratch[0], cal.nops * scale)
        with torch.cuda.stream(P):
            out.fill_(0x5A5A)
            ready = torch.cuda.Event()
            ready.record(P)
        pending_before = not ready.query()
        host_ms = _timed(lambda: eng.synth_device(SEED, clips, n, out.data_ptr(), offsets=offsets, stream=handle))
        with torch.cuda.stream(P):
            got = out.clone()
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        assert np.array_equal(g, host), "%d of %d samples wrong, %d of them the sentinel" % (
            (g != host).sum(), g.size, ((g != host) & (g == 0x5A5A)).sum())
        return _waited(cal, scale, pending_before, host_ms)

    _run(case)


# ---- more than one stream at work ------------------------------------------------------------------

def test_mixed_order_side_stream_then_host_search(rig):
    """tfp_fingerprint_device on side stream A, not synchronised; a host-form search on the engine's own
    stream; then the consumer on A. The search returns while A's producer is still pending: on another
    hardware queue than A's, that is (test_foreign_side_stream_is_not_waited_for), so a run whose window was
    closed takes the next side stream of torch's pool."""
    torch, eng, d, cal = rig.torch, rig.engine, rig.data, rig.cal
    b = d.enrol
    _enrol(rig)
    p = rig.tfp_lib.params(1, 0.001)
    frames = _query_frames(d.queries.db)
    eng.search_batch(frames, d.queries.foff, p)
    real, decoy = torch.from_numpy(b.real).cuda(), torch.from_numpy(b.decoy).cuda()
    plan = eng.plan(b.off)

    def case(scale):
        A, handle = _stream(torch, "side")
        pcm = decoy.clone()
        micro = _sentinel(torch, (b.nframes, 2), torch.int32)
        torch.cuda.synchronize()
        ready = _pending(torch, cal, A, scale, [(pcm, real)])
        eng.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), 0, handle)
        open_after_call = not ready.query()
        res, _ = eng.search_batch(frames, d.queries.foff, p)
        with torch.cuda.stream(A):
            got = micro.clone()
        open_after_clones = not ready.query()
        torch.cuda.synchronize()
        _assert_host_results(rig, res, 1, 0.001)
        _assert_micro(got, b)
        return _async_window(open_after_call, open_after_clones)

    try:
        _run(case)
    finally:
        eng.index_clear()


def test_two_calls_on_two_side_streams(rig):
    """tfp_fingerprint_device on side stream A, then at once on side stream B, into different outputs; each
    stream has its own pending producer (B's real input is A's decoy and the other way round)."""
    torch, eng, cal, b = rig.torch, rig.engine, rig.cal, rig.data.enrol
    A, ha = _stream(torch, "side")
    B, hb = _stream(torch, "side")
    assert ha != hb
    first, second = torch.from_numpy(b.real).cuda(), torch.from_numpy(b.decoy).cuda()
    other = Bag()  # the batch as B sees it
    other.micro, other.decoy_micro = b.decoy_micro, b.micro
    plan = eng.plan(b.off)

    def case(scale):
        pcm_a, pcm_b = second.clone(), first.clone()
        micro_a = _sentinel(torch, (b.nframes, 2), torch.int32)
        micro_b = _sentinel(torch, (b.nframes, 2), torch.int32)
        torch.cuda.synchronize()
        ready_a = _pending(torch, cal, A, scale, [(pcm_a, first)], row=0)
        ready_b = _pending(torch, cal, B, scale, [(pcm_b, second)], row=1)
        eng.fingerprint_device(plan, pcm_a.data_ptr(), micro_a.data_ptr(), 0, ha)
        eng.fingerprint_device(plan, pcm_b.data_ptr(), micro_b.data_ptr(), 0, hb)
        open_after_call = not ready_a.query() and not ready_b.query()
        with torch.cuda.stream(A):
            got_a = micro_a.clone()
        with torch.cuda.stream(B):
            got_b = micro_b.clone()
        open_after_clones = not ready_a.query() and not ready_b.query()
        torch.cuda.synchronize()
        _assert_micro(got_a, b, "stream A:")
        _assert_micro(got_b, other, "stream B:")
        return _async_window(open_after_call, open_after_clones)

    _run(case)


def test_foreign_side_stream_is_not_waited_for(rig):
    """stream = NULL orders the call against the null stream alone: the input is produced and the output
    consumed on the default stream while a torch side stream is busy with an unrelated, longer delay.
    The result is right, the call returns and the consumer is queued while that side stream is busy, and
    the side stream is still busy once the default stream has finished.

    The last holds only for a side stream on another hardware queue than the null stream's and the engine
    stream's: HIP maps its streams onto a few hardware queues (4 by default) in turn, and two streams on
    one queue run in submission order whatever their events say (measured with torch ops alone: every
    fourth side stream delays the default stream this way). So the case runs over consecutive side
    streams of torch's pool until one is still busy; a wait in the engine itself, a device synchronise or a
    wait for every stream, would find none of the eight."""
    torch, eng, cal, b = rig.torch, rig.engine, rig.cal, rig.data.enrol
    D, _ = _stream(torch, "default")
    real, decoy = torch.from_numpy(b.real).cuda(), torch.from_numpy(b.decoy).cuda()
    plan = eng.plan(b.off)
    seen = Bag()

    def case(scale):
        pcm = decoy.clone()
        micro = _sentinel(torch, (b.nframes, 2), torch.int32)
        torch.cuda.synchronize()
        _queue_delay(torch, seen.F, cal.scratch[1], 4 * cal.nops * scale)
        busy = torch.cuda.Event()
        busy.record(seen.F)
        ready = _pending(torch, cal, D, scale, [(pcm, real)], row=0)
        eng.fingerprint_device(plan, pcm.data_ptr(), micro.data_ptr(), 0, 0)
        open_after_call = not ready.query() and not busy.query()
        got = micro.clone()
        open_after_clones = not ready.query() and not busy.query()
        D.synchronize()
        seen.busy_after = not busy.query()
        torch.cuda.synchronize()
        _assert_micro(got, b)
        return _async_window(open_after_call, open_after_clones)

    for _ in range(8):
        seen.F, _ = _stream(torch, "side")
        _run(case)
        if seen.busy_after:
            return
    pytest.fail("the call or its consumer waited for each of 8 unrelated side streams")
