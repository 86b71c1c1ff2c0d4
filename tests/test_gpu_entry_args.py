"""What every search entry point answers to a bad call: the return code and tfp_engine_last_error's
text, one table row per (entry point, bad call), and per entry point one row with two faults at once,
which pins the order of its checks. The frames and the PCM entry point of a form share their rows; only
the offsets and the missing-data messages name the source."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, CAPACITY = -1, -5
SPC, HOP, WINDOW, WHOP = 16000, 256, 8, 4
MONO = {"frames": "qoffsets not monotone", "pcm": "offsets not monotone"}
NODATA = {"frames": "frames is NULL", "pcm": "samples are NULL"}

# the arguments after (engine, data, offsets, n[, sample_rate], params) of each form's entry points
FORMS = {
    "ranked": ("tfp_search_ranked{}_batch", ["k", "out", "counts"]),
    "scoped": ("tfp_search_scoped{}_batch", ["scopes", "k", "out", "counts"]),
    "aligned": ("tfp_search_aligned{}_batch", ["k", "out", "align", "counts"]),
    "census": ("tfp_census{}_batch", ["scopes", "nbins", "hist", "need"]),
    "sliding": ("tfp_search_sliding{}_batch", ["window", "hop", "scopes", "k", "out", "counts", "cap", "nw"]),
    "sliding_aligned": ("tfp_search_sliding_aligned{}_batch",
                        ["window", "hop", "scopes", "k", "out", "counts", "align", "cap", "nw"]),
    "occurrences": ("tfp_search_occurrences{}_batch",
                    ["window", "hop", "scopes", "k", "max_gap", "min_hits", "occ", "ocap", "nocc"]),
    "align": ("tfp_align_batch", ["ids", "k", "align"]),
    "align_sliding": ("tfp_align_sliding_batch", ["window", "hop", "ids", "k", "align", "cap", "nw"]),
    "trace": ("tfp_trace_batch", ["reqs", "nreqs", "max_gap", "tout"]),
}
FRAMES_ONLY = ("align", "align_sliding", "trace")
SLIDING = ("sliding", "sliding_aligned", "occurrences", "align_sliding", "trace")

# (form, bad call) -> (code, text); "mono" / "nodata" stand for the source's own message. A bad call is a
# dict of overrides of the valid call; "mono": the offsets fall, "nodata": the data pointer is NULL. With
# n = -1 the falling offsets must go unnoticed: a count below 0 is refused without reading them.
K0, K33, COEFS3, WIN0 = {"k": 0}, {"k": 33}, {"coefs": 3}, {"window": 0}
BADSCOPE = {"scopes": [-1, -2]}
TABLE = [
    ("ranked", {"mono": 1}, ARG, "mono"),
    ("ranked", {"nodata": 1}, ARG, "nodata"),
    ("ranked", K0, ARG, "ranked search: k = 0 outside [1, 32]"),
    ("ranked", K33, ARG, "ranked search: k = 33 outside [1, 32]"),
    ("ranked", COEFS3, ARG, "ranked search: coefs outside [1, 2]"),
    ("ranked", {"out": None}, ARG, "ranked search: bad query count or NULL output"),
    ("ranked", {"counts": None}, ARG, "ranked search: bad query count or NULL output"),
    ("ranked", {"n": -1}, ARG, "ranked search: bad query count or NULL output"),
    ("ranked", {"k": 0, "mono": 1}, ARG, "ranked search: k = 0 outside [1, 32]"),
    ("ranked", {"coefs": 3, "nodata": 1}, ARG, "ranked search: coefs outside [1, 2]"),
    ("scoped", {"mono": 1}, ARG, "mono"),
    ("scoped", {"nodata": 1}, ARG, "nodata"),
    ("scoped", K0, ARG, "ranked search: k = 0 outside [1, 32]"),
    ("scoped", K33, ARG, "ranked search: k = 33 outside [1, 32]"),
    ("scoped", COEFS3, ARG, "ranked search: coefs outside [1, 2]"),
    ("scoped", BADSCOPE, ARG, "scoped search: scope -2 of query 1"),
    ("scoped", {"scopes": None}, ARG, "scoped search: scopes is NULL"),
    ("scoped", {"out": None}, ARG, "ranked search: bad query count or NULL output"),
    ("scoped", {"n": -1}, ARG, "ranked search: bad query count or NULL output"),
    ("scoped", {"scopes": [-1, -2], "mono": 1}, ARG, "scoped search: scope -2 of query 1"),
    ("scoped", {"scopes": [-1, -2], "k": 0}, ARG, "ranked search: k = 0 outside [1, 32]"),
    ("aligned", {"mono": 1}, ARG, "mono"),
    ("aligned", {"nodata": 1}, ARG, "nodata"),
    ("aligned", K0, ARG, "ranked search: k = 0 outside [1, 32]"),
    ("aligned", K33, ARG, "ranked search: k = 33 outside [1, 32]"),
    ("aligned", COEFS3, ARG, "ranked search: coefs outside [1, 2]"),
    ("aligned", {"align": None}, ARG, "aligned search: NULL output"),
    ("aligned", {"out": None}, ARG, "ranked search: bad query count or NULL output"),
    ("aligned", {"n": -1}, ARG, "ranked search: bad query count or NULL output"),
    ("aligned", {"align": None, "k": 0}, ARG, "aligned search: NULL output"),
    ("census", {"mono": 1}, ARG, "mono"),
    ("census", {"nodata": 1}, ARG, "nodata"),
    ("census", COEFS3, ARG, "census: coefs outside [1, 2]"),
    ("census", BADSCOPE, ARG, "census: scope -2 of query 1"),
    ("census", {"nbins": 32}, CAPACITY, "census: 32 bins, the longest query needs 33"),
    ("census", {"hist": None}, ARG, "census: hist is NULL"),
    ("census", {"need": None}, ARG, "census: bad query count or NULL need_bins"),
    ("census", {"n": -1}, ARG, "census: bad query count or NULL need_bins"),
    ("census", {"mono": 1, "nbins": 32}, ARG, "mono"),
    ("census", {"nodata": 1, "nbins": 32}, ARG, "nodata"),
    ("census", {"scopes": [-1, -2], "mono": 1}, ARG, "census: scope -2 of query 1"),
    ("sliding", {"mono": 1}, ARG, "mono"),
    ("sliding", {"nodata": 1}, ARG, "nodata"),
    ("sliding", K0, ARG, "sliding search: k = 0 outside [1, 32]"),
    ("sliding", K33, ARG, "sliding search: k = 33 outside [1, 32]"),
    ("sliding", COEFS3, ARG, "sliding search: coefs outside [1, 2]"),
    ("sliding", BADSCOPE, ARG, "sliding search: scope -2 of recording 1"),
    ("sliding", WIN0, ARG, "sliding search: window = 0, hop = 4"),
    ("sliding", {"cap": 1}, CAPACITY, "sliding search: 2 windows, room for 1"),
    ("sliding", {"out": None}, ARG, "sliding search: NULL output"),
    ("sliding", {"counts": None}, ARG, "sliding search: NULL output"),
    ("sliding", {"nw": None}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("sliding", {"n": -1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("sliding", {"n": -1, "mono": 1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("sliding", {"mono": 1, "k": 0}, ARG, "mono"),
    ("sliding", {"window": 0, "k": 0}, ARG, "sliding search: window = 0, hop = 4"),
    ("sliding", {"cap": 1, "out": None}, CAPACITY, "sliding search: 2 windows, room for 1"),
    ("sliding_aligned", {"mono": 1}, ARG, "mono"),
    ("sliding_aligned", {"nodata": 1}, ARG, "nodata"),
    ("sliding_aligned", K0, ARG, "sliding search: k = 0 outside [1, 32]"),
    ("sliding_aligned", K33, ARG, "sliding search: k = 33 outside [1, 32]"),
    ("sliding_aligned", COEFS3, ARG, "sliding search: coefs outside [1, 2]"),
    ("sliding_aligned", BADSCOPE, ARG, "sliding search: scope -2 of recording 1"),
    ("sliding_aligned", WIN0, ARG, "sliding search: window = 0, hop = 4"),
    ("sliding_aligned", {"cap": 1}, CAPACITY, "sliding search: 2 windows, room for 1"),
    ("sliding_aligned", {"out": None}, ARG, "sliding search: NULL output"),
    ("sliding_aligned", {"align": None}, ARG, "sliding aligned search: NULL output"),
    ("sliding_aligned", {"n": -1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("sliding_aligned", {"n": -1, "mono": 1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("sliding_aligned", {"align": None, "nodata": 1}, ARG, "sliding aligned search: NULL output"),
    ("sliding_aligned", {"align": None, "cap": 1}, CAPACITY, "sliding search: 2 windows, room for 1"),
    ("sliding_aligned", {"mono": 1, "window": 0}, ARG, "mono"),
    ("occurrences", {"mono": 1}, ARG, "mono"),
    ("occurrences", {"nodata": 1}, ARG, "nodata"),
    ("occurrences", K0, ARG, "occurrence search: k = 0 outside [1, 32]"),
    ("occurrences", K33, ARG, "occurrence search: k = 33 outside [1, 32]"),
    ("occurrences", COEFS3, ARG, "sliding search: coefs outside [1, 2]"),
    ("occurrences", BADSCOPE, ARG, "sliding search: scope -2 of recording 1"),
    ("occurrences", WIN0, ARG, "sliding search: window = 0, hop = 4"),
    ("occurrences", {"max_gap": -1}, ARG, "occurrence search: max_gap = -1, min_hits = 2"),
    ("occurrences", {"min_hits": 0}, ARG, "occurrence search: max_gap = 2, min_hits = 0"),
    ("occurrences", {"nocc": None}, ARG, "occurrence search: NULL noccurrences"),
    ("occurrences", {"occ": None}, ARG, "occurrence search: NULL output"),
    ("occurrences", {"n": -1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("occurrences", {"n": -1, "mono": 1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("occurrences", {"k": 0, "mono": 1}, ARG, "occurrence search: k = 0 outside [1, 32]"),
    ("occurrences", {"mono": 1, "window": 0}, ARG, "mono"),
    ("align", {"mono": 1}, ARG, "mono"),
    ("align", {"nodata": 1}, ARG, "nodata"),
    ("align", K0, ARG, "aligned search: k = 0 outside [1, 32]"),
    ("align", K33, ARG, "aligned search: k = 33 outside [1, 32]"),
    ("align", COEFS3, ARG, "aligned search: coefs outside [1, 2]"),
    ("align", {"align": None}, ARG, "aligned search: bad query count or NULL output"),
    ("align", {"ids": None}, ARG, "aligned search: clip_ids is NULL"),
    ("align", {"ids": None, "mono": 1}, ARG, "aligned search: clip_ids is NULL"),
    ("align_sliding", {"mono": 1}, ARG, "mono"),
    ("align_sliding", {"nodata": 1}, ARG, "nodata"),
    ("align_sliding", K0, ARG, "sliding search: k = 0 outside [1, 32]"),
    ("align_sliding", K33, ARG, "sliding search: k = 33 outside [1, 32]"),
    ("align_sliding", {"align": None}, ARG, "sliding search: NULL output"),
    ("align_sliding", {"n": -1, "mono": 1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("align_sliding", COEFS3, ARG, "sliding search: coefs outside [1, 2]"),
    ("align_sliding", WIN0, ARG, "sliding search: window = 0, hop = 4"),
    ("align_sliding", {"cap": 1}, CAPACITY, "sliding search: 2 windows, room for 1"),
    ("align_sliding", {"ids": None}, ARG, "sliding search: NULL output"),
    ("align_sliding", {"n": -1}, ARG, "sliding search: bad recording count or NULL nwindows"),
    ("align_sliding", {"mono": 1, "cap": 1}, ARG, "mono"),
    ("trace", {"mono": 1}, ARG, "mono"),
    ("trace", {"nodata": 1}, ARG, "nodata"),
    ("trace", COEFS3, ARG, "trace: coefs outside [1, 2]"),
    ("trace", {"max_gap": -1}, ARG, "trace: max_gap = -1"),
    ("trace", {"tout": None}, ARG, "trace: bad count or NULL array"),
    ("trace", {"n": -1}, ARG, "trace: bad count or NULL array"),
    ("trace", {"coefs": 3, "mono": 1}, ARG, "trace: coefs outside [1, 2]"),
]


@pytest.fixture(scope="module")
def world(tfp_lib):
    """An engine over 6 synthetic clips of 2 s, and the valid call's arguments per source."""
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    T = tfp_lib
    eng = T.Engine(0)
    pcm = T.synth_pcm(0x51A7E, range(6), SPC)
    fr = eng.fingerprint_batch(pcm.reshape(-1), np.arange(7) * SPC)
    nf = T.frame_count(SPC)
    uuids = ["00000000-0000-4000-8000-%012d" % c for c in range(6)]
    for c in range(6):
        eng.index_add(uuids[c], fr["m1"][c * nf:(c + 1) * nf], fr["m2"][c * nf:(c + 1) * nf])
    eng.index_set_scope(uuids, [c % 2 for c in range(6)])
    eng.index_commit()

    def source(cuts):
        q = np.ascontiguousarray(np.concatenate([pcm[c, a:a + n] for c, a, n in cuts]))
        off = np.concatenate([[0], np.cumsum([n for _, _, n in cuts])]).astype(np.int64)
        qfr = eng.fingerprint_batch(q, off)
        qoff = np.concatenate([[0], np.cumsum([T.frame_count(n) for _, _, n in cuts])]).astype(np.int64)
        return {"pcm": (q, off), "frames": (qfr, qoff)}

    w = {"T": T, "eng": eng,
         "queries": source([(1, 0, HOP + 1), (2, 10 * HOP, 8000)]),              # 2 and 32 frames
         "recordings": source([(1, 5 * HOP, 7 * HOP), (3, 5 * HOP, 12 * HOP)])}  # window - 1 and window + hop frames
    yield w
    eng.close()


def _call(w, form, src, bad):
    """The valid call of `form` from source `src` with `bad` laid over it: (code, text, outputs)."""
    T, eng = w["T"], w["eng"]
    name, tail = FORMS[form]
    data, off = w["recordings" if form in SLIDING else "queries"][src]
    keep = [data, off]  # (arrays referenced until the call returns)
    if bad.get("mono"):
        off = off.copy()
        off[1], off[2] = off[2], off[1] - 1
        keep.append(off)
    p = T.params(bad.get("coefs", 1), 1.0)  # (1 dB: the least at which the synthetic clips' own cuts hit them)
    nwin = 64
    from tiresias_amd._lib import Alignment, Candidate, Occurrence
    v = {"k": 3, "window": WINDOW, "hop": WHOP, "scopes": np.array([0, -1], np.int32),
         "out": (Candidate * (nwin * 33))(), "counts": (C.c_int32 * nwin)(), "align": (Alignment * (nwin * 33))(),
         "nbins": 33, "hist": np.full((2, 40), -77, np.int32), "need": C.c_int32(-9), "cap": 2, "nw": C.c_int64(-9),
         "max_gap": 2, "min_hits": 2, "occ": (Occurrence * 256)(), "ocap": 256, "nocc": C.c_int64(-9),
         "ids": np.full(nwin * 33, -1, np.int32), "reqs": np.array([[1, 3, 0, 0]], np.int32), "nreqs": 1,
         "tout": np.zeros((1, 6), np.int32)}
    for key, val in bad.items():
        if key in v:
            v[key] = None if val is None else np.array(val, np.int32) if key == "scopes" else val
    args = [eng.handle, None if bad.get("nodata") else data.ctypes.data, off.ctypes.data, bad.get("n", 2)]
    if src == "pcm":
        args.append(8000)
    args.append(C.byref(p))
    for a in tail:
        x = v[a]
        if isinstance(x, np.ndarray):
            x = x.ctypes.data
        elif isinstance(x, (C.c_int32, C.c_int64)):
            x = C.byref(x)
        args.append(x)
    L = T.lib()
    scope = C.c_int32()
    assert L.tfp_index_scope(eng.handle, b"no such clip", C.byref(scope)) == -4  # another text in the error slot
    rc = getattr(L, name.format("_pcm" if src == "pcm" else ""))(*args)
    return rc, eng.last_error(), v


def _sources(form):
    return ("frames",) if form in FRAMES_ONLY else ("frames", "pcm")


def test_the_valid_call_of_every_entry_point_passes(world):
    for form in FORMS:
        for src in _sources(form):
            rc, text, v = _call(world, form, src, {})
            assert rc == 0, (form, src, text)
            if "nw" in FORMS[form][1]:
                assert v["nw"].value == 2
            if form == "census":
                assert v["need"].value == 33
            if form == "occurrences":
                assert v["nocc"].value >= 1


def test_table(world):
    wrong = []
    for form, bad, code, text in TABLE:
        for src in _sources(form):
            want = {"mono": MONO, "nodata": NODATA}[text][src] if text in ("mono", "nodata") else text
            rc, got, v = _call(world, form, src, bad)
            print(form, src, bad, rc, repr(got))
            if (rc, got) != (code, want):
                wrong.append((form, src, bad, rc, got))
            # the counts a capacity error still reports
            if "cap" in bad and not bad.get("mono") and (rc != CAPACITY or v["nw"].value != 2):
                wrong.append((form, src, bad, "nwindows", v["nw"].value))
            if form == "census" and bad.get("nbins") and not (bad.get("mono") or bad.get("nodata")):
                if rc != CAPACITY or v["need"].value != 33 or not (v["hist"] == -77).all():
                    wrong.append((form, src, bad, "need_bins", v["need"].value))
    assert not wrong, wrong
    assert {f for f, *_ in TABLE} == set(FORMS)


def test_occurrence_list_one_too_small(world):
    """TFP_E_CAPACITY with the count the list needs, as the sliding forms report their windows."""
    for src in ("frames", "pcm"):
        rc, _, v = _call(world, "occurrences", src, {})
        n = v["nocc"].value
        assert rc == 0 and n >= 1
        rc, text, v = _call(world, "occurrences", src, {"ocap": n - 1})
        assert (rc, text, v["nocc"].value) == (CAPACITY, "occurrence search: %d occurrences, room for %d" % (n, n - 1), n)
