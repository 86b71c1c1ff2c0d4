"""Shared by the catalog-neighbour tests: a catalog held beside the engine, the brute-force reference
(ranked_util.brute_force on the named clip's converted rows with its own row deleted, align_util.brute_force
per row) and the engine's own composition (rows read back, scoped search at k + 1, align_batch)."""
import contextlib

import numpy as np

import align_util as A
import ranked_util as R

ANY = -1
NULL = R.NULL


class Catalog:
    """uuids[c] with rows (m1[c], m2[c]) and scope[c]; removed clips leave `alive`."""

    def __init__(self, uuids, rows, scopes=None):
        self.uuids = list(uuids)
        self.m1 = [np.asarray(a, np.int64) for a, _ in rows]
        self.m2 = [np.asarray(b, np.int64) for _, b in rows]
        self.scope = list(scopes) if scopes is not None else [0] * len(self.uuids)
        self.alive = [True] * len(self.uuids)

    def enrol(self, eng):
        eng.index_clear()
        fo = np.concatenate([[0], np.cumsum([len(a) for a in self.m1])])
        eng.index_add_batch(self.uuids, fo, np.concatenate(self.m1 + [np.zeros(0, np.int64)]).astype(np.int32),
                            np.concatenate(self.m2 + [np.zeros(0, np.int64)]).astype(np.int32))
        eng.index_set_scope(self.uuids, self.scope)

    def add(self, eng, uuid, m1, m2, scope=0):
        eng.index_add(uuid, np.asarray(m1, np.int32), np.asarray(m2, np.int32))
        eng.index_set_scope([uuid], [scope])
        self.uuids.append(uuid)
        self.m1.append(np.asarray(m1, np.int64))
        self.m2.append(np.asarray(m2, np.int64))
        self.scope.append(scope)
        self.alive.append(True)

    def q(self, c):
        """The frame values of clip c's rows: m / 1e6, None (-inf) for a stored NULL."""
        conv = lambda v: [None if x == NULL else int(x) / 1e6 for x in v]
        return conv(self.m1[c]), conv(self.m2[c])

    def table(self, scope):
        """(clip, m1, m2) over the live clips of the scope."""
        keep = [c for c in range(len(self.uuids)) if self.alive[c] and (scope == ANY or self.scope[c] == scope)]
        if not keep:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
        return (np.concatenate([np.full(len(self.m1[c]), c, np.int64) for c in keep]),
                np.concatenate([self.m1[c] for c in keep]), np.concatenate([self.m2[c] for c in keep]))


def ref_rows(oracle, cat, c, coefs, tol, low, high, scope=ANY, key=None):
    """Every row of clip c's result query in the scope, its own row deleted: [(uuid, count), ...].
    key (uuid -> tie key): tied counts by key descending instead of uuid descending."""
    clip, m1, m2 = cat.table(scope)
    q1, q2 = cat.q(c)
    rows = [r for r in R.brute_force(oracle, cat.uuids, clip, m1, m2, q1, q2, coefs, tol, low, high) if r[0] != cat.uuids[c]]
    if key:
        rows.sort(key=lambda r: (r[1], key[r[0]]), reverse=True)
    return rows


def ref_align(oracle, cat, c, uuid, coefs, tol, low, high):
    b = cat.uuids.index(uuid)
    q1, q2 = cat.q(c)
    return A.brute_force(oracle, cat.m1[b], cat.m2[b], q1, q2, coefs, tol, low, high)


def got_rows(res):
    return [R.pairs(r["neighbours"]) for r in res]


@contextlib.contextmanager
def cached_boxes():
    """ranked_util.frame_box memoised while the block runs: both brute forces ask the oracle for the same
    frame's box once per clip and parameter set instead of once per candidate (the values are the oracle's)."""
    real, memo = R.frame_box, {}

    def frame_box(oracle, *args):
        if args not in memo:
            memo[args] = real(oracle, *args)
        return memo[args]

    R.frame_box = frame_box
    try:
        yield
    finally:
        R.frame_box = real


def read_frames(eng, uuid):
    """The clip's rows read back from the engine, as the frames a caller would build from them."""
    m1, m2 = eng.index_rows(uuid)
    conv = lambda v: [None if x == NULL else int(x) / 1e6 for x in v]
    return R.frames_from_q(conv(m1), conv(m2))


def composed_batch(eng, uuids, frames, p, k, scopes):
    """The caller's composition for many clips in one batch per step: scoped search at k + 1, the own row
    dropped, align_batch on what remains. [(rows, alignments), ...]."""
    fr = np.concatenate(frames)
    qoff = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    found = eng.search_scoped_batch(fr, qoff, p, scopes, k + 1)
    rows = [[r for r in found[i] if r["audio_uuid"] != uuids[i]][:k] for i in range(len(uuids))]
    ids = [[r["clip_id"] for r in rs] + [-1] * (k - len(rs)) for rs in rows]
    al = eng.align_batch(fr, qoff, p, np.asarray(ids, np.int32).reshape(-1), k)
    return [(R.pairs(rows[i]), [A.four(a) for a in al[i][:len(rows[i])]]) for i in range(len(uuids))]


def composed(eng, uuid, p, k, scope):
    """The caller's composition for one clip: (rows, alignments, frame count)."""
    m1, m2 = eng.index_rows(uuid)
    fr = R.frames_from_q([None if x == NULL else int(x) / 1e6 for x in m1], [None if x == NULL else int(x) / 1e6 for x in m2])
    qoff = [0, len(fr)]
    rows = [r for r in eng.search_scoped_batch(fr, qoff, p, [scope], k + 1)[0] if r["audio_uuid"] != uuid][:k]
    ids = [r["clip_id"] for r in rows] + [-1] * (k - len(rows))
    al = eng.align_batch(fr, qoff, p, ids, k)[0][:len(rows)]
    return R.pairs(rows), [A.four(a) for a in al], len(fr)


def check(eng, oracle, tfp_lib, cat, names, coefs, tol, k, scopes=None, low=-1, high=-1, aligned=True, compose=True, key=None,
          align_rows=None):
    """index_neighbours for the named clip indices against the reference (and the composition); returns the result."""
    p = tfp_lib.params(coefs, tol, low, high)
    res = eng.index_neighbours([cat.uuids[c] for c in names], p, k, scopes, aligned)
    assert len(res) == len(names)
    for i, c in enumerate(names):
        sc = ANY if scopes is None else scopes[i]
        exp = ref_rows(oracle, cat, c, coefs, tol, low, high, sc, key)[:k]
        got = R.pairs(res[i]["neighbours"])
        assert got == exp, (cat.uuids[c], coefs, tol, k, sc, got, exp)
        assert res[i]["frame_count"] == len(cat.m1[c])
        if aligned:
            for r, row in enumerate(res[i]["neighbours"][:align_rows]):
                assert A.four(row) == ref_align(oracle, cat, c, row["audio_uuid"], coefs, tol, low, high), (cat.uuids[c], r)
        if compose and k <= 31 and key is None:
            rows, al, nf = composed(eng, cat.uuids[c], p, k, sc)
            assert got == rows and nf == res[i]["frame_count"]
            if aligned:
                assert [A.four(row) for row in res[i]["neighbours"]] == al
    return res
