"""Shared by the aligned trailing-window tests of live calls (tfp_live_window_aligned and its group form):
the comparison of a call's rows with tfp_live_window's definition (live_window_util.definition_rows) and of
every row's alignment with tfp_align_batch on exactly the kept frame values of the channel's window."""
import numpy as np

import align_util as A
import live_util as L
import live_window_util as W

ZERO = dict.fromkeys(A.FIELDS, 0)
ASTAT_KEYS = ("inplace_calls", "general_calls", "pairs")


def expected_aligns(tfp, engine, lv, p, rows, first_frames, k, ids=None):
    """tfp_align_batch (on `engine`) of every channel's window [first, F) as lv.frames reads it out against
    the clips of its rows (ids: per channel the rows' clip ids on `engine`; None: the rows' own clip_id)."""
    n = lv.nchannels
    fr = [lv.frames(c, first_frames[c]) for c in range(n)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in fr])])
    frames = np.concatenate(fr) if off[-1] else np.zeros(1, tfp.FRAME_DTYPE)
    flat = np.full(n * k, -1, np.int32)
    for c in range(n):
        got = [r["clip_id"] for r in rows[c]] if ids is None else ids[c]
        flat[c * k:c * k + len(got)] = got
    return engine.align_batch(frames, off, p, flat, k)


def check_aligned(tfp, owner, lv, p, scopes, k, window, where=None, engine=None, ids_of=None):
    """Asks for the aligned window and asserts rows, frame counts and first frames against the definition,
    every alignment against tfp_align_batch, and zeros past each channel's rows. engine: the engine that
    aligns (owner when it is one); ids_of(rows of a channel) -> their clip ids on that engine."""
    rows, al, fc, ff = lv.window_aligned(p, scopes, k, window)
    exp, efc, eff = W.definition_rows(tfp, owner, lv, p, scopes, k, window)
    assert fc == efc and ff == eff, (where, fc, efc, ff, eff)
    for c in range(lv.nchannels):
        assert rows[c] == exp[c], (where, c, lv.samples(c))
        L.assert_twins_tie(rows[c])
    ids = None if ids_of is None else [ids_of(rows[c]) for c in range(lv.nchannels)]
    ea = expected_aligns(tfp, engine or owner, lv, p, rows, ff, k, ids)
    for c in range(lv.nchannels):
        assert len(al[c]) == k
        for r in range(k):
            if r < len(rows[c]):
                assert al[c][r] == ea[c][r], (where, c, r, rows[c][r], al[c][r], ea[c][r])
                assert 1 <= al[c][r]["aligned_count"] <= rows[c][r]["match_count"], (where, c, r)
                assert 0 <= al[c][r]["first_frame"] <= al[c][r]["last_frame"] < fc[c], (where, c, r)
            else:
                assert al[c][r] == ZERO, (where, c, r)
    return rows, al, fc, ff
