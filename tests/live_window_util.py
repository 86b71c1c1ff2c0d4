"""Shared by the trailing-window tests of live calls (tfp_live_window, tfp_group_live_window): two-part
calls over live_util's DB, the comparison of a window call's rows with the scoped search of exactly
the kept frame values of each channel's window (the contract of tiresias_fp.h), and a frame-by-frame
mirror of the count rows' ranges from which the expected tfp_live_window_stats follow."""
import numpy as np

import live_util as L
import ranked_util as R

T = 160  # a 20 ms SLIN tick at 8 kHz
TICKS = 40
WSTAT_KEYS = ("slid_calls", "general_calls", "rebuilds", "frames_added", "frames_removed", "rows_restarted")
# (first clip, its offset, second clip, its offset) per channel: the second clip lies in another scope
# than the first (clip c is in scope c % 3); with live_util.SCOPES8 channels 0, 1, 4 and 7 start inside
# their own context's clip and leave it, 3, 5 and 6 rank every clip
PARTS = ((L.TWIN[0], 1024, 7, 333), (7, 333, 12, 1), (12, 1, 20, 777), (20, 777, 33, 2049), (33, 2049, 4, 100),
         (3, 1535, 8, 64), (10, 257, 11, 511), (13, 900, 14, 3))
SILENT = 5            # this channel has 10 frames of silence between its parts
PART1 = 15 * 256      # samples of the first part


def two_part_calls(db, nsamples=TICKS * T):
    """8 calls of nsamples samples: a window of one clip, then a window of a clip of another scope."""
    src = []
    for c, (a, ao, b, bo) in enumerate(PARTS):
        n1 = PART1 - (5 * 256 if c == SILENT else 0)
        gap = 10 * 256 if c == SILENT else 0
        x = np.concatenate([db["pcm"][a][ao:ao + n1], np.zeros(gap, np.int16), db["pcm"][b][bo:bo + nsamples - n1 - gap]])
        assert len(x) == nsamples
        src.append(x)
    return np.stack(src)


def window_of(tfp, S, window):
    """(first, F) of a channel with S samples."""
    F = tfp.frame_count(S) if S else 0
    return max(0, F - window), F


class Rows:
    """A mirror of the engine's bookkeeping, not an independent check of it: the count rows' ranges as the
    header states them, kept as sets of frames, with live_window_plan's restart rule restated, so that a
    test can say which tfp_live_window_stats it expects after each call. The rule itself, and the bound
    on the frames visited, are checked against brute-force set differences by
    tests/native/check_live_window.cpp."""

    def __init__(self, nch):
        self.rng = [set() for _ in range(nch)]
        self.stale = True
        self.exp = dict.fromkeys(WSTAT_KEYS, 0)

    def reset(self, c=None):
        for i in (range(len(self.rng)) if c is None else [c]):
            self.exp["frames_removed"] += len(self.rng[i])
            self.rng[i] = set()

    def restamp(self):
        """The next slid call finds the table's stamp changed."""
        self.stale = True

    def slid(self, samples, window):
        """A call served from the table: every row moves to its target [first, Ff)."""
        if self.stale:
            self.reset()
            self.exp["rebuilds"] += 1
            self.stale = False
        for c, S in enumerate(samples):
            F, Ff = (S + 255) // 256, S // 256
            tgt, row = set(range(max(0, F - window), Ff)), self.rng[c]
            leaving, entering = len(row - tgt), len(tgt - row)
            if not row or len(tgt) < leaving + entering:  # restart
                self.exp["frames_added"] += len(tgt)
                self.exp["frames_removed"] += len(row)
                self.exp["rows_restarted"] += 1 if (tgt or row) else 0
            else:
                self.exp["frames_added"] += entering
                self.exp["frames_removed"] += leaving
            self.rng[c] = tgt
        self.exp["slid_calls"] += 1

    def general(self):
        self.exp["general_calls"] += 1

    def check(self, lv, where=None):
        st = lv.window_stats()
        assert st == self.exp, (where, st, self.exp)
        assert st["frames_added"] - st["frames_removed"] == sum(len(r) for r in self.rng), where


def definition_rows(tfp, owner, lv, p, scopes, k, window):
    """search_scoped_batch on exactly the kept frame values of every channel's window, one query per channel."""
    n = lv.nchannels
    fr, ff, fc = [], [], []
    for c in range(n):
        first, F = window_of(tfp, lv.samples(c), window)
        f = lv.frames(c, first)
        assert len(f) == F - first and (not len(f) or (f["frame_idx"][0] == first and f["frame_idx"][-1] == F - 1))
        fr.append(f)
        ff.append(first)
        fc.append(F - first)
    off = np.concatenate([[0], np.cumsum(fc)])
    frames = np.concatenate(fr) if off[-1] else np.zeros(1, tfp.FRAME_DTYPE)
    return owner.search_scoped_batch(frames, off, p, [-1] * n if scopes is None else scopes, k), fc, ff


def check_window(tfp, owner, lv, p, scopes, k, window, where=None):
    """Asks for the window rows and asserts rows, frame counts and first frames against the definition."""
    rows, fc, ff = lv.window(p, scopes, k, window)
    exp, efc, eff = definition_rows(tfp, owner, lv, p, scopes, k, window)
    assert fc == efc and ff == eff, (where, fc, efc, ff, eff)
    for c in range(lv.nchannels):
        assert rows[c] == exp[c], (where, c, lv.samples(c))
        L.assert_twins_tie(rows[c])
    return rows


def oracle_window_rows(oracle, db, h, tol, scope, k, window, coefs=1):
    """live_util.oracle_rows with a slice: the CPU oracle's fingerprint of the call so far, its frames
    [first, F), then the brute-force count over the scope's clips."""
    import scoped_util as S
    if not len(h):
        return []
    _, qdb, _ = oracle.fingerprint(h)
    first = max(0, len(qdb) - window)
    sub = (db["uuids"], db["clip"], db["m1"], db["m2"]) if scope < 0 else S.restrict(db, scope)
    return R.brute_force(oracle, *sub, list(qdb[first:, 0]), list(qdb[first:, 1]), coefs, tol, -1, -1, limit=k)


def push_all(lv, hist, blk, nsamples=None, law=None, codes=None):
    """An ingest-only push of blk (channel c takes nsamples[c]); extends hist."""
    n = [blk.shape[1]] * len(hist) if nsamples is None else list(nsamples)
    for c in range(len(hist)):
        hist[c] = np.concatenate([hist[c], blk[c, :n[c]]])
    if law is None:
        assert lv.push(blk, None, nsamples=nsamples) is None
    else:
        assert lv.push_g711(codes, law, None, nsamples=nsamples) is None
