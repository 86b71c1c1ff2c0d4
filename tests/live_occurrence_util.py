"""Shared by the occurrence tests of live calls (tfp_live_occurrences and its group form): a synthetic DB of
clips whose sound, and with it the frame key, varies every two frames, and the reference of every check, composed only of entry points
that have parity tests of their own.

Ref mirrors a live object's lists in Python. After each call it reads every channel's kept frames
(tfp_live_frames), takes the expected rows and alignments as live_window_aligned_util computes them
(tfp_search_scoped_batch + tfp_align_batch on the window's frames), applies the header's offer rule to its
own lists, traces every list entry with tfp_trace_batch over all F frames, thins them by occurrence_util's
rule, and compares out, dropped, tfp_live_tracks and frames_traced exactly (integers: no tolerance)."""
import numpy as np

import live_window_aligned_util as WA
import live_window_util as W
import occurrence_util as O

T = 160  # a 20 ms SLIN tick at 8 kHz
SEED = 0x0CC5
NFRAMES = (40, 57, 64, 75, 88, 101, 113, 120)  # the clips' lengths in frames
LATE = 7                                        # enrolled after the first build: it lies in the index delta
SCOPE_OF = (0, 1, 0, 0, 1, 2, 2, 2)              # three contexts of two or three clips
TRACK_KEYS = ("clip_id", "start", "windows") + O.TRACE_KEYS
OSTAT_KEYS = ("calls", "tracks_added", "tracks_dropped", "frames_traced", "retraces")


def uuid_of(c):
    return "%08x-3333-4000-8000-%012x" % (0x10000000 * (c % 7) + c, c)


def _symbol(kind, n, rs):
    """512 samples whose frame value lies a little above an integer key of its own (measured with the CPU oracle:
    16.2, 17.2, 18.05 and 19.3), so that at tolerance 0.45 a frame hits the rows of its own kind only."""
    t = np.arange(n)
    if kind == 0:
        return rs.uniform(-1, 1, n) * 30000.0
    if kind == 1:
        return rs.uniform(-1, 1, n) * 300.0
    if kind == 2:
        return np.sin(2 * np.pi * 700.0 * t / 8000.0) * 20000.0
    return np.sin(2 * np.pi * 1500.0 * t / 8000.0) * 200.0


def clip_pcm(tfp, c):
    """A pseudo-random sequence over four kinds of sound, one kind per two 256-sample frames (loud noise, soft
    noise, a loud 700 Hz tone, a soft 1,500 Hz tone: frame keys 16, 17, 18 and 19). The keys fall in an
    aperiodic pattern, so a 48-frame stretch of a clip lies on one diagonal of it with every frame hitting
    and on every other diagonal, and in every other clip, with about one frame in four."""
    rs = np.random.RandomState(100 + c)
    kinds = rs.randint(0, 4, (NFRAMES[c] + 1) // 2)
    x = np.concatenate([_symbol(k, 512, rs) for k in kinds])[:NFRAMES[c] * 256]
    return np.round(x).astype(np.int16)


def build_db(tfp, owner, fingerprinter=None):
    """The 8 clips on `owner` (an Engine or a Group): 7, an index build (a search), then clip LATE, which an
    engine with the index delta enabled keeps in its delta. Returns pcm, uuids and each clip's rows."""
    fp = fingerprinter or owner
    pcm = [clip_pcm(tfp, c) for c in range(len(NFRAMES))]
    uuids = [uuid_of(c) for c in range(len(NFRAMES))]
    nrows = {}
    first = [c for c in range(len(NFRAMES)) if c != LATE]
    for c in first + [LATE]:
        if c == LATE:  # the index is built before the last clip arrives
            owner.index_commit()
            fr = fp.fingerprint(pcm[0][:2560])
            owner.search_scoped_batch(fr, [0, len(fr)], tfp.params(1, 0.45), [-1], 1)
        fr = fp.fingerprint(pcm[c])
        assert len(fr) == NFRAMES[c]
        owner.index_add(uuids[c], fr["m1"], fr["m2"])
        nrows[uuids[c]] = NFRAMES[c]
    owner.index_set_scope(uuids, list(SCOPE_OF))
    return {"pcm": pcm, "uuids": uuids, "nrows": nrows, "scope": dict(zip(uuids, SCOPE_OF))}


def noise(tfp, n, clip=900, level=400.0):
    x = tfp.synth_pcm(SEED, [clip], n)[0].astype(np.float64)
    return np.round(x * (level / np.abs(x).max())).astype(np.int16)


def occurrences_of_tracks(tracks, min_hits):
    """occurrence_util.occurrences_of_rows from its grouping on, over list entries: tracks = [(channel, uuid,
    clip_id, s, windows, trace tuple)], already filtered by enrolment and scope."""
    groups = {}
    for c, uuid, cid, s, n, t in tracks:
        if t[3] >= min_hits:
            groups.setdefault((c, uuid, cid), []).append((s, n, t))
    out = []
    for (c, uuid, cid), cands in groups.items():
        kept = []
        for s, n, t in sorted(cands, key=lambda x: (-x[2][3], -x[1], x[0])):
            if not any(t[4] <= q[2][5] and q[2][4] <= t[5] for q in kept):
                kept.append((s, n, t))
        for s, n, t in kept:
            row = dict(zip(O.OCC_KEYS, (c, uuid, s, t[4], t[5], t[3], t[1], t[0], n)))
            row["clip_id"] = cid
            out.append(row)
    out.sort(key=lambda o: o["audio_uuid"], reverse=True)
    out.sort(key=lambda o: (o["recording"], o["first_frame"], -o["hits"]))  # (stable: equal keys stay uuid-descending)
    return out


class Ref:
    """The running lists and the expected counters of one live object. engine: the engine the reference's
    searches, alignments and traces run on (every clip of db enrolled on it under the same uuids; a group's
    test keeps a single engine beside the group). enrolled: the uuids now in the index, kept by the test."""

    def __init__(self, tfp, engine, lv, db, own=True):
        """own: lv is `engine`'s own live object (else a group's: clip ids are not compared, they number
        shards there, and the per-shard counters are left to the caller)."""
        self.tfp, self.engine, self.lv, self.db = tfp, engine, lv, db
        self.lists = [[] for _ in range(lv.nchannels)]  # entries: dict(uuid, clip_id, s, windows, done)
        self.enrolled = set(db["uuids"])
        self.nrows = dict(db["nrows"])
        self.scope = dict(db["scope"])
        self.stamp = None
        self.exp = dict.fromkeys(OSTAT_KEYS, 0)
        self.own = own

    def reset(self, c=None):
        for i in (range(len(self.lists)) if c is None else [c]):
            self.lists[i] = []

    def call(self, p, scopes, k, window, max_gap, min_hits, max_tracks, where=None):
        """One tfp_live_occurrences call checked against the composition."""
        tfp, lv, n = self.tfp, self.lv, self.lv.nchannels
        got, dropped = lv.occurrences(p, scopes, k, window, max_gap, min_hits, max_tracks)
        # the index as the call saw it, before the reference's own searches touch it: every build, merge and
        # delta update is a new index version (the stamp's first field)
        version = (tuple(self.engine.index_build_stats()), self.engine.index_delta_stats()[0])
        self.exp["calls"] += 1
        # step 1: the rows and alignments of the trailing window, by their definitions
        rows, fc, ff = W.definition_rows(tfp, self.engine, lv, p, scopes, k, window)
        al = WA.expected_aligns(tfp, self.engine, lv, p, rows, ff, k)
        # step 2: the offer rule
        exp_dropped = [0] * n
        for c in range(n):
            for r, row in enumerate(rows[c]):
                if al[c][r]["aligned_count"] < 1:
                    continue
                s = ff[c] - al[c][r]["offset"]
                hit = [t for t in self.lists[c] if t["uuid"] == row["audio_uuid"] and t["s"] == s]
                if hit:
                    hit[0]["windows"] += 1
                elif len(self.lists[c]) < max_tracks:
                    self.lists[c].append(dict(uuid=row["audio_uuid"], clip_id=row["clip_id"], s=s, windows=1, done=None))
                    self.exp["tracks_added"] += 1
                else:
                    exp_dropped[c] += 1
                    self.exp["tracks_dropped"] += 1
        assert dropped == exp_dropped, (where, dropped, exp_dropped)
        # step 3: a changed stamp starts every summary again; the tracks of removed clips leave; every entry
        # traced over all F frames
        stamp = (version, p.coefs, p.tolerance, p.freq_ignore_low, p.freq_ignore_high, max_gap)
        if stamp != self.stamp:
            if any(t["done"] is not None for lst in self.lists for t in lst):
                self.exp["retraces"] += 1
            for lst in self.lists:
                for t in lst:
                    t["done"] = None
            self.stamp = stamp
        frames, off, reqs = [], [0], []
        for c in range(n):
            self.lists[c] = [t for t in self.lists[c] if t["uuid"] in self.enrolled]
            f = lv.frames(c, 0)
            frames.append(f)
            off.append(off[-1] + len(f))
            S = lv.samples(c)
            F, Ff = (S + 255) // 256, S // 256
            assert len(f) == F
            for t in self.lists[c]:
                reqs.append((c, t["clip_id"], t["s"]))
                N = self.nrows[t["uuid"]]
                lo, end = max(0, t["s"]), min(Ff, t["s"] + N)
                tail_in = S % 256 != 0 and lo <= Ff < t["s"] + N
                beg = lo if t["done"] is None else max(t["done"], lo)
                if end > beg:
                    self.exp["frames_traced"] += end - beg
                    t["done"] = end
                elif tail_in and t["done"] is None:
                    # The header counts a retrace for "a call that had a summary to start again". A track
                    # whose span holds only the tail so far has been answered by the kernel, which stored its
                    # summary (of no final frame yet): it has one, so a later stamp change counts. This is the
                    # contract's rule restated, and the one place where "has a summary" is not "has folded a frame".
                    t["done"] = lo
        allf = np.concatenate(frames) if off[-1] else np.zeros(1, tfp.FRAME_DTYPE)
        tr = self.engine.trace_batch(allf, off, p, reqs, max_gap)
        i = 0
        tracks = []
        for c in range(n):
            mine = lv.tracks(c)
            assert len(mine) == len(self.lists[c]), (where, c, mine, self.lists[c])
            for t, m in zip(self.lists[c], mine):
                e = dict(clip_id=t["clip_id"], start=t["s"], windows=t["windows"], **tr[i])
                keys = TRACK_KEYS if self.own else TRACK_KEYS[1:]
                assert {q: m[q] for q in keys} == {q: e[q] for q in keys}, (where, c, m, e)
                scope = -1 if scopes is None else scopes[c]
                if scope == -1 or self.scope[t["uuid"]] == scope:
                    tracks.append((c, t["uuid"], t["clip_id"], t["s"], t["windows"], tuple(tr[i][q] for q in O.TRACE_KEYS)))
                i += 1
        # step 4
        exp = occurrences_of_tracks(tracks, min_hits)
        flat = [o for c in range(n) for o in got[c]]
        if not self.own:
            flat, exp = O.strip(flat), O.strip(exp)
        assert flat == exp, (where, flat, exp)
        if self.own:
            st = lv.occurrence_stats()
            assert st == self.exp, (where, st, self.exp)
        return got, dropped
