"""Shared by the occurrence-search tests: the fixture (tests/golden/occurrence_cases.json) and a numpy
reference of the diagonal trace and of the occurrence list, over one align_util.hit_matrix of the whole
recording with a clip (bool [F, N]: hit(x, j)).

trace_of_hits(hits, s, max_gap): the clip laid with its frame 0 at recording frame s covers the frames
[max(0, s), min(F, s + N)); the hitting frames x (hits[x, x - s]) fall into segments, maximal runs with
x' - x - 1 <= max_gap; the result is (overlap, hits, segments, seg_hits, seg_first, seg_last), the best
segment having the most hits, the earliest of equals; all but overlap 0 without a hit.

occurrences_of_rows(rows, hop, trace, min_hits): steps 2-5 of include/tiresias_fp.h's occurrence search
over the rows (recording, audio_uuid, window index, offset) of a sliding aligned search."""
import functools
import json
import os

import numpy as np

import ranked_util as R

INT32_MAX = 2 ** 31 - 1
TRACE_KEYS = ("overlap", "hits", "segments", "seg_hits", "seg_first", "seg_last")
OCC_KEYS = ("recording", "audio_uuid", "clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap",
            "windows")


def trace_of_hits(hits, s, max_gap, more=False):
    """With more, also whether several segments have the best one's hits (the earliest is named)."""
    F, N = hits.shape
    lo, hi = max(0, s), min(F, s + N)
    overlap = max(0, hi - lo)
    t, tie = (overlap, 0, 0, 0, 0, 0), False
    if overlap:
        x = np.arange(lo, hi)
        xs = x[hits[x, x - s]]
        if len(xs):
            cuts = np.nonzero(np.diff(xs) - 1 > max_gap)[0] + 1
            starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts, [len(xs)]])
            size = ends - starts
            b = int(np.argmax(size))  # (argmax: the first, so the earliest, of equals)
            t = (overlap, len(xs), len(starts), int(size[b]), int(xs[starts[b]]), int(xs[ends[b] - 1]))
            tie = int((size == size[b]).sum()) > 1
    return (t, tie) if more else t


def candidates_of_rows(rows, hop):
    """{(recording, uuid, s): windows} of rows = [(recording, uuid, w, offset), ...]."""
    named = {}
    for r, uuid, w, offset in rows:
        key = (r, uuid, w * hop - offset)
        named[key] = named.get(key, 0) + 1
    return named


def occurrences_of_rows(rows, hop, trace, min_hits):
    """The occurrence dicts (OCC_KEYS) in output order; trace(recording, uuid, s) -> trace_of_hits' tuple at the
    call's max_gap."""
    named = candidates_of_rows(rows, hop)
    groups = {}
    for (r, uuid, s), n in named.items():
        t = trace(r, uuid, s)
        if t[3] >= min_hits:
            groups.setdefault((r, uuid), []).append((s, n, t))
    out = []
    for (r, uuid), cands in groups.items():
        kept = []
        for s, n, t in sorted(cands, key=lambda c: (-c[2][3], -c[1], c[0])):
            if not any(t[4] <= k[2][5] and k[2][4] <= t[5] for k in kept):
                kept.append((s, n, t))
        out += [dict(zip(OCC_KEYS, (r, uuid, s, t[4], t[5], t[3], t[1], t[0], n))) for s, n, t in kept]
    out.sort(key=lambda o: o["audio_uuid"], reverse=True)
    out.sort(key=lambda o: (o["recording"], o["first_frame"], -o["hits"]))  # (stable: equal keys stay uuid-descending)
    return out


def strip(occ):
    """Occurrence dicts without clip_id (an engine's clip number, a group's shard)."""
    return [{k: o[k] for k in OCC_KEYS} for o in occ]


@functools.lru_cache(maxsize=None)
def load_occurrences():
    """[(scenario name, query index, window, hop, context or -1, [(max_gap, min_hits, traces, occurrences)])]:
    traces = [(uuid, s, windows, (overlap, hits, segments, seg_hits, seg_first, seg_last))], occurrences = OCC_KEYS
    dicts of recording 0."""
    with open(os.path.join(R.GOLDEN, "occurrence_cases.json")) as f:
        doc = json.load(f)
    scen, _ = R.load_cases()
    out = []
    for name, qi, window, hop, ctx, per in doc["cases"]:
        u = scen[name]["uuids"]
        out.append((name, qi, window, hop, ctx,
                    [(g, m, [(u[c], s, n, tuple(t)) for c, s, n, *t in tr],
                      [dict(zip(OCC_KEYS, (0, u[c], s, *rest))) for c, s, *rest in occ]) for g, m, tr, occ in per]))
    return out
