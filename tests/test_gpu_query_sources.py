"""Every search form that takes frames or samples gives the same answer from both: the PCM entry point
on the samples, and the frames entry point on tfp_fingerprint_batch's frames of those samples, agree field
for field (rows, counts, alignments, census bins and need_bins, windows, occurrences) and take the same
form's path (*_stats), on a main index, with a live delta, without queries and on an empty index."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPC, HOP, WINDOW, WHOP, K, ANY = 16000, 256, 8, 4, 4, -1
UUIDS = ["00000000-0000-4000-8000-%012d" % c for c in range(7)]
# one batch: no sample, one sample, one hop + 1 samples, and 1 s cut from clip 2
QUERIES = [(0, 0, 0), (0, 7, 1), (1, 0, HOP + 1), (2, 10 * HOP, 8000)]
QSCOPES = [ANY, 0, 1, 0]
# one frame short of a window, no sample, and window + hop frames (2 windows) cut from clip 3
RECORDINGS = [(1, 5 * HOP, (WINDOW - 1) * HOP), (0, 0, 0), (3, 5 * HOP, (WINDOW + WHOP) * HOP)]
RSCOPES = [ANY, 0, 1]


@pytest.fixture(scope="module")
def clips(tfp_lib):
    """7 synthetic clips of 2 s at 8 kHz and their frames (6 are indexed, the 7th joins as the delta)."""
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    pcm = tfp_lib.synth_pcm(0x51A7E, range(7), SPC)
    with tfp_lib.Engine(0) as eng:
        fr = eng.fingerprint_batch(pcm.reshape(-1), np.arange(8) * SPC)
    return pcm, fr


def _add(eng, T, clips, ids):
    nf = T.frame_count(SPC)
    for c in ids:
        eng.index_add(UUIDS[c], clips[1]["m1"][c * nf:(c + 1) * nf], clips[1]["m2"][c * nf:(c + 1) * nf])
    eng.index_set_scope([UUIDS[c] for c in ids], [c % 2 for c in ids])


def _source(eng, T, pcm, cuts):
    """The cuts as one batch, from both sources: (samples, sample offsets), (frames, frame offsets)."""
    q = np.ascontiguousarray(np.concatenate([pcm[c, a:a + n] for c, a, n in cuts] + [np.zeros(0, np.int16)]))
    off = np.concatenate([[0], np.cumsum([n for _, _, n in cuts])]).astype(np.int64)
    qoff = np.concatenate([[0], np.cumsum([T.frame_count(n) for _, _, n in cuts])]).astype(np.int64)
    return (q, off), (eng.fingerprint_batch(q, off), qoff)


def _census(eng, T, name, data, off, head, p, scopes, nbins):
    """The census through ctypes: (hist, need_bins)."""
    nq = len(off) - 1
    hist, need = np.full((max(nq, 1), nbins), -77, np.int32), C.c_int32(-9)
    sc = np.ascontiguousarray(scopes, np.int32)
    eng._chk(getattr(T.lib(), name)(eng.handle, data.ctypes.data, off.ctypes.data, nq, *head, C.byref(p), sc.ctypes.data,
                                    nbins, hist.ctypes.data, C.byref(need)))
    return hist[:nq].tolist(), need.value


def _stats(eng):
    return {f: getattr(eng, f + "_stats")() for f in ("rank", "scope", "census", "slide", "align", "slide_align", "trace")}


def _moved(before, after):
    """The counters that changed, as {form.counter: increment}; the scope table's builds are left out:
    the first scoped call after an index update builds it, whichever source asks."""
    return {f"{f}.{k}": after[f][k] - before[f][k] for f in after for k in after[f]
            if after[f][k] != before[f][k] and k != "table_builds"}


def _both(eng, T, pcm, p, queries=QUERIES, qscopes=QSCOPES, recordings=RECORDINGS, rscopes=RSCOPES):
    """Every form from both sources: {form: answer} (asserted equal), and {form: the counters it moved}."""
    (q, off), (qfr, qoff) = _source(eng, T, pcm, queries)
    (r, roff), (rfr, rqoff) = _source(eng, T, pcm, recordings)
    nbins = max([T.frame_count(n) for _, _, n in queries], default=0) + 1
    forms = {
        "ranked": (lambda: eng.search_ranked_batch(qfr, qoff, p, K), lambda: eng.search_ranked_pcm_batch(q, off, p, K)),
        "scoped": (lambda: eng.search_scoped_batch(qfr, qoff, p, qscopes, K),
                   lambda: eng.search_scoped_pcm_batch(q, off, p, qscopes, K)),
        "aligned": (lambda: eng.search_aligned_batch(qfr, qoff, p, K), lambda: eng.search_aligned_pcm_batch(q, off, p, K)),
        "census": (lambda: _census(eng, T, "tfp_census_batch", qfr, qoff, (), p, qscopes, nbins),
                   lambda: _census(eng, T, "tfp_census_pcm_batch", q, off, (8000,), p, qscopes, nbins)),
        "sliding": (lambda: eng.search_sliding_batch(rfr, rqoff, p, WINDOW, WHOP, K, rscopes),
                    lambda: eng.search_sliding_pcm_batch(r, roff, p, WINDOW, WHOP, K, rscopes)),
        "sliding_aligned": (lambda: eng.search_sliding_aligned_batch(rfr, rqoff, p, WINDOW, WHOP, K, rscopes),
                            lambda: eng.search_sliding_aligned_pcm_batch(r, roff, p, WINDOW, WHOP, K, rscopes)),
        "occurrences": (lambda: eng.search_occurrences_batch(rfr, rqoff, p, WINDOW, WHOP, K, 2, 2, rscopes),
                        lambda: eng.search_occurrences_pcm_batch(r, roff, p, WINDOW, WHOP, K, 2, 2, rscopes)),
    }
    answers, moved = {}, {}
    for form, calls in forms.items():
        got = []
        for call in calls:
            before = _stats(eng)
            got.append((call(), _moved(before, _stats(eng))))
        print(form, got[0][1], got[1][1])
        assert got[0][0] == got[1][0], form  # field for field
        assert got[0][1] == got[1][1], form  # the same path
        answers[form], moved[form] = got[0]
    return answers, moved


def _rows(answer):
    return sum(len(rows) for per in answer for rows in per)


# (coefs, tolerance) -> the form each family takes on a populated index. The search truncates a frame's
# value to whole dB before it adds the tolerance (fp_handler.c:290) and the synthetic clips peak a little
# under 17 dB, so a tolerance of 1 dB is the least at which their own cuts hit them. 9.0 lies outside
# delta_tol_ok: the sliding forms then take the general form, the ranked forms' vote kernels serve any
# tolerance.
TOL = 1.0
PATHS = {(1, TOL): ("vote", "vote"), (2, TOL): ("general", "general"), (1, 9.0): ("vote", "general")}


def _check_paths(moved, ranked, slid, windows=2):
    assert moved["ranked"] == {f"rank.{ranked}_batches": 1}
    assert moved["scoped"] == {f"scope.{ranked}_batches": 1}
    assert moved["aligned"] == {f"rank.{ranked}_batches": 1, "align.batches": 1, "align.pairs": moved["aligned"]["align.pairs"]}
    assert moved["census"] == {f"census.{ranked}_batches": 1}
    assert moved["sliding"] == {f"slide.{slid}_batches": 1, "slide.windows": windows}
    sa = moved["sliding_aligned"]
    assert sa["slide.windows"] == windows and sa[f"slide.{slid}_batches"] == 1 and sa["slide_align.batches"] == 1
    oc = moved["occurrences"]
    assert {k: v for k, v in oc.items() if not k.startswith("trace.")} == sa and oc["trace.batches"] == 1


@pytest.mark.parametrize("coefs,tol", list(PATHS))
def test_main_index(tfp_lib, clips, coefs, tol):
    T = tfp_lib
    with T.Engine(0) as eng:
        _add(eng, T, clips, range(6))
        eng.index_commit()
        answers, moved = _both(eng, T, clips[0], T.params(coefs, tol))
        _check_paths(moved, *PATHS[(coefs, tol)])
        assert answers["ranked"][0] == [] and _rows([answers["ranked"]]) > 0
        assert all(int(r["audio_uuid"][-1]) % 2 == 1 for r in answers["scoped"][2])
        hist, need = answers["census"]
        assert need == T.frame_count(8000) + 1 and [sum(h) for h in hist] == [6, 3, 3, 3]
        assert [len(per) for per in answers["sliding"]] == [0, 0, 2]
        assert _rows(answers["sliding"]) > 0 and answers["occurrences"][2] and not answers["occurrences"][0]


def test_live_delta(tfp_lib, clips, monkeypatch):
    """One clip added after the commit lies in the index delta; the coefs = 1 forms serve it from there."""
    T = tfp_lib
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the delta at any index size
    with T.Engine(0) as eng:
        _add(eng, T, clips, range(6))
        eng.index_commit()
        _add(eng, T, clips, [6])
        queries = QUERIES + [(6, 20 * HOP, 4000)]
        recordings = RECORDINGS + [(6, 9 * HOP, (WINDOW + WHOP) * HOP)]
        answers, moved = _both(eng, T, clips[0], T.params(1, TOL), queries, QSCOPES + [ANY], recordings, RSCOPES + [ANY])
        assert eng.index_delta_stats()[1] == 1  # still beside the index
        _check_paths(moved, "vote", "vote", windows=4)
        assert UUIDS[6] in [r["audio_uuid"] for r in answers["ranked"][4]]  # the delta's clip is found
        assert UUIDS[6] in [r["audio_uuid"] for w in answers["sliding_aligned"][3] for r in w]
        assert sum(answers["census"][0][4]) == 7
        answers2, moved2 = _both(eng, T, clips[0], T.params(2, TOL), queries, QSCOPES + [ANY], recordings, RSCOPES + [ANY])
        _check_paths(moved2, "general", "general", windows=4)
        assert UUIDS[6] in [r["audio_uuid"] for r in answers2["ranked"][4]]


@pytest.mark.parametrize("coefs", [1, 2])
def test_no_query_and_empty_index(tfp_lib, clips, coefs):
    T = tfp_lib
    p = T.params(coefs, TOL)
    with T.Engine(0) as eng:
        # an empty index: every form answers and nothing is found. The vote forms return before they count a
        # batch, the general forms count theirs; no alignment and no trace is launched
        answers, moved = _both(eng, T, clips[0], p)
        assert _rows([answers["ranked"]]) == 0 and _rows(answers["sliding"]) == 0 and answers["occurrences"] == [[], [], []]
        assert answers["census"] == ([[0] * 33] * 4, 33)
        assert [len(per) for per in answers["sliding_aligned"]] == [0, 0, 2]
        slid = {"slide.general_batches": 1, "slide.windows": 2}
        assert moved == ({f: {} for f in moved} if coefs == 1 else {
            "ranked": {"rank.general_batches": 1}, "scoped": {"scope.general_batches": 1},
            "aligned": {"rank.general_batches": 1}, "census": {"census.general_batches": 1}, "sliding": slid,
            "sliding_aligned": slid, "occurrences": slid})
    with T.Engine(0) as eng:
        # nq = 0 / nrec = 0 over staged clips: no answer, no counter, and the index is not built
        _add(eng, T, clips, range(6))
        answers, moved = _both(eng, T, clips[0], p, [], [], [], [])
        assert answers == {"ranked": [], "scoped": [], "aligned": [], "census": ([], 1), "sliding": [], "sliding_aligned": [],
                           "occurrences": []}
        assert all(m == {} for m in moved.values())
        assert eng.index_build_stats() == (0, 0)


def test_zero_frame_batch_and_staged_clips(tfp_lib, clips):
    """A batch whose every query has no frame, over clips staged but not committed: which entry points
    build the index (tfp_index_build_stats). Ranked search from frames does, from samples it returns before;
    the census does from both, since bin 0 needs the scopes' populations."""
    T = tfp_lib
    p = T.params(1, TOL)
    none, zeros = np.zeros(0, np.int16), np.zeros(3, np.int64)
    calls = {
        "ranked frames": (lambda e: e.search_ranked_batch(np.zeros(0, T.FRAME_DTYPE), zeros, p, K), [[], []], (1, 0)),
        "ranked pcm": (lambda e: e.search_ranked_pcm_batch(none, zeros, p, K), [[], []], (0, 0)),
        "census frames": (lambda e: e.census_batch(np.zeros(0, T.FRAME_DTYPE), zeros, p, [ANY, 1]).tolist(), [[6], [3]], (1, 0)),
        "census pcm": (lambda e: e.census_pcm_batch(none, zeros, p, [ANY, 1]).tolist(), [[6], [3]], (1, 0)),
    }
    for name, (call, want, builds) in calls.items():
        with T.Engine(0) as eng:
            _add(eng, T, clips, range(6))
            before = eng.index_build_stats()
            got = call(eng)
            after = eng.index_build_stats()
            print(name, got, before, after)
            assert got == want and before == (0, 0) and after == builds, name
