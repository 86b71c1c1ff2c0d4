"""Shared by the live-call tests (tfp_live_*, tfp_group_live_*): a small scoped DB of synthetic clips,
calls that play windows of them, and the comparison of a push's rows with the scoped search of each
channel's call so far (tfp_search_scoped_pcm_batch on the prefixes: the contract of tiresias_fp.h)."""
import numpy as np

import ranked_util as R
import scoped_util as S

SEED = 0x11FE
NCLIPS = 40
TWIN = (5, 38)  # byte-identical clips under different uuids, both in scope 2
ROWLESS = 39    # enrolled with NULL rows only: it never has a row
STAT_KEYS = ("incremental_pushes", "general_pushes", "rebuilds", "frames_fingerprinted", "frames_added")


def clip_len(c):
    return 8000 + 197 * c  # 1-2 s, odd lengths


def uuid_of(c):
    return "%08x-2222-4000-8000-%012x" % (c * 2654435761 % 2**32, c)  # uuid order is not enrolment order


def clip_pcm(tfp, c):
    src = TWIN[0] if c == TWIN[1] else c
    return tfp.synth_pcm(SEED, [src], clip_len(src))[0]


def build_db(tfp, owner):
    """Enrols the DB into an emptied Engine or Group: clip c in scope c % 3 (scoped_util's assignment).
    Returns the scenario as scoped_util.restrict / ranked_util.brute_force read it, plus the clips' PCM."""
    pcms = [clip_pcm(tfp, c) for c in range(NCLIPS)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in pcms])])
    fr = owner.fingerprint_batch(np.concatenate(pcms), off)
    foff = np.concatenate([[0], np.cumsum([tfp.frame_count(len(x)) for x in pcms])])
    m1, m2 = fr["m1"].copy(), fr["m2"].copy()
    m1[foff[ROWLESS]:foff[ROWLESS + 1]] = R.NULL
    m2[foff[ROWLESS]:foff[ROWLESS + 1]] = R.NULL
    uuids = [uuid_of(c) for c in range(NCLIPS)]
    owner.index_clear()
    owner.index_add_batch(uuids, foff, m1, m2)
    owner.index_set_scope(uuids, [c % S.CONTEXTS for c in range(NCLIPS)])
    return {"uuids": uuids, "clip": np.repeat(np.arange(NCLIPS), np.diff(foff)), "m1": m1.astype(np.int64),
            "m2": m2.astype(np.int64), "pcm": pcms}


def calls(tfp, db, nsamples):
    """8 calls of nsamples samples: windows of clips at odd sample offsets (one of the twin clips, on a
    hop boundary, among them), a window that starts late in its clip, noise, and silence."""
    src = [db["pcm"][c][o:o + nsamples] for c, o in ((TWIN[0], 1024), (7, 333), (12, 1), (20, 777), (33, 2049), (3, 1535))]
    src.append(tfp.synth_pcm(0xBEEF, [0], nsamples)[0])
    src.append(np.zeros(nsamples, np.int16))
    assert all(len(x) == nsamples for x in src)
    return np.stack(src)


SCOPES8 = [2, 1, S.UNUSED_SCOPE, -1, 0, -1, -1, 1]  # the calls' scopes: own context, another's, none's, ANY


def prefix_rows(owner, hist, p, scopes, k):
    """The scoped search of every channel's samples so far, one query per channel."""
    off = np.concatenate([[0], np.cumsum([len(h) for h in hist])])
    pcm = np.concatenate(hist) if off[-1] else np.zeros(1, np.int16)
    return owner.search_scoped_pcm_batch(pcm, off, p, scopes, k)


def check_push(tfp, owner, lv, hist, blk, p, scopes, k, nsamples=None, where=None):
    """Pushes blk (channel c takes nsamples[c]), extends hist, and asserts rows, counts and frame counts."""
    n = [blk.shape[1]] * len(hist) if nsamples is None else list(nsamples)
    for c in range(len(hist)):
        hist[c] = np.concatenate([hist[c], blk[c, :n[c]]])
    rows, fc = lv.push(blk, p, scopes, k, nsamples)
    exp = prefix_rows(owner, hist, p, [-1] * len(hist) if scopes is None else scopes, k)
    assert fc == [tfp.frame_count(len(h)) for h in hist], where
    for c in range(len(hist)):
        assert rows[c] == exp[c], (where, c, len(hist[c]))
        if not len(hist[c]):
            assert rows[c] == []
        assert_twins_tie(rows[c])
    return rows


def assert_twins_tie(rows):
    """The byte-identical clips have equal counts: where both are among the rows, the greater uuid comes first."""
    at = {r["audio_uuid"]: (i, r["match_count"]) for i, r in enumerate(rows)}
    lo, hi = sorted(uuid_of(c) for c in TWIN)
    if lo in at:
        assert hi in at and at[hi][0] < at[lo][0] and at[hi][1] == at[lo][1], rows


def oracle_rows(oracle, db, h, tol, scope, k, coefs=1):
    """The CPU oracle's rows of one call so far: its fingerprint, then the brute-force count over the
    scope's clips (scoped_util.restrict, ranked_util.brute_force)."""
    if not len(h):
        return []
    _, qdb, _ = oracle.fingerprint(h)
    sub = (db["uuids"], db["clip"], db["m1"], db["m2"]) if scope < 0 else S.restrict(db, scope)
    return R.brute_force(oracle, *sub, list(qdb[:, 0]), list(qdb[:, 1]), coefs, tol, -1, -1, limit=k)
