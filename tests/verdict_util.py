"""Shared by the live-verdict tests (tfp_live_verdict, tfp_group_live_verdict): a DB of noise clips
whose level moves from hop to hop, calls that play them, and the verdict restated from the rule in
tiresias_fp.h over the CPU oracle's brute-force counts.

live_util's synthetic clips tie widely at coefs = 1 (their first coefficient hardly moves), so no
call over them is ever decided early. Here every 256-sample hop of a clip has a level of its own,
drawn per clip from kinds 80 dB apart end to end (see clip_pcm: 40 dB of level moves the first value by
less than 1, so it would not change the truncated max1 keys), so the keys differ from frame to frame
and from clip to clip. The DB's rows are the CPU oracle's fingerprints: everything the tests need of the data is
asserted on the oracle alone (assert_data), before any GPU call."""
import functools

import numpy as np

import ranked_util as R

SEED = 0x5EED1
NCLIPS = 24
CONTEXTS = 3
CLIP_SAMPLES = 16128  # 63 hops, about 2 s
TWIN = (4, 19)        # byte-identical clips under different uuids, both in scope 1
ROWLESS = 11          # enrolled with NULL rows only (scope 2)
REMOVED = 23          # removed after enrolment; the greatest uuid of all, in scope 2
LONE = 9              # the only clip of scope LONE_SCOPE
LONE_SCOPE = 5
ZLEAD, ZRIVAL = 17, 14  # the only clips of scope ZSCOPE: ZRIVAL has the greater uuid and never scores on ZLEAD's audio
ZSCOPE = 6
TOL = 0.45
T = 160               # a 20 ms tick at 8 kHz


def uuid_of(c):
    # uuid order is not enrolment order; the removed clip is the greatest, the twins are apart
    return "%08x-5555-4000-8000-%012x" % (0xFFFFFFFF if c == REMOVED else c * 2654435761 % 2**32, c)


def scope_of(c):
    return LONE_SCOPE if c == LONE else ZSCOPE if c in (ZLEAD, ZRIVAL) else c % CONTEXTS


# The first fingerprint value moves slowly with level (about 16.2 at full scale, 17.1 at amplitude 300,
# 18.1 at amplitude 1, 19.0 for a pure tone), and a coefs = 1 frame matches the rows within the tolerance
# of its truncated value. So a hop is drawn from four kinds whose frames match rows of their own kind
# at TOL: loud, middle and faint noise (80 dB apart end to end) and a tone. A clip draws its hops from
# its own one or two kinds, in an order of its own.
KINDS = 4


def clip_kinds(c):
    src = TWIN[0] if c == TWIN[1] else c
    fixed = {LONE: (1,), ZLEAD: (0,), ZRIVAL: (3,), 6: (0, 1), 7: (1, 2), 2: (0,), 12: (2, 3), 3: (1,), REMOVED: (0, 1, 2, 3)}
    if src in fixed:
        return fixed[src]
    rng = np.random.default_rng(SEED * 31 + src)
    return tuple(sorted(rng.choice(KINDS, size=int(rng.integers(1, 3)), replace=False).tolist()))


@functools.lru_cache(maxsize=None)
def clip_pcm(c):
    src = TWIN[0] if c == TWIN[1] else c
    rng = np.random.default_rng(SEED + src)
    hops = CLIP_SAMPLES // 256
    kinds = np.asarray(clip_kinds(src))
    seq = kinds[rng.integers(0, len(kinds), hops)]
    amp = np.array([20000.0, 300.0, 1.0, 0.0])[seq] * 10.0 ** (rng.uniform(-3.0, 3.0, hops) / 20.0)
    x = rng.standard_normal(CLIP_SAMPLES) * np.repeat(amp, 256)
    t = np.arange(CLIP_SAMPLES)
    x += np.repeat(seq == 3, 256) * 8000.0 * np.sin(2 * np.pi * 2000.0 * t / 8000.0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _db(oracle):
    pcms = [clip_pcm(c) for c in range(NCLIPS)]
    m1, m2, clip = [], [], []
    for c, x in enumerate(pcms):
        _, _, micro = oracle.fingerprint(x)
        a, b = micro[:, 0].astype(np.int64), micro[:, 1].astype(np.int64)
        if c == ROWLESS:
            a[:], b[:] = R.NULL, R.NULL
        m1.append(a), m2.append(b), clip.append(np.full(len(a), c))
    return {"uuids": [uuid_of(c) for c in range(NCLIPS)], "clip": np.concatenate(clip), "m1": np.concatenate(m1),
            "m2": np.concatenate(m2), "pcm": pcms, "scope": [scope_of(c) for c in range(NCLIPS)]}


def db(oracle):
    return _db(oracle)


def enrol(owner, d, removed=True, only=None):
    """The DB into an emptied Engine or Group (only: a subset of clips), its scopes set; then REMOVED removed."""
    owner.index_clear()
    ids = list(range(NCLIPS)) if only is None else list(only)
    rows = [np.nonzero(d["clip"] == c)[0] for c in ids]
    foff = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    sel = np.concatenate(rows)
    owner.index_add_batch([d["uuids"][c] for c in ids], foff, d["m1"][sel].astype(np.int32), d["m2"][sel].astype(np.int32))
    owner.index_set_scope([d["uuids"][c] for c in ids], [d["scope"][c] for c in ids])
    if removed and REMOVED in ids:
        owner.index_remove(d["uuids"][REMOVED])


def candidates(d, scope, alive):
    """The clips a verdict ranks: enrolled, not removed, in scope, with at least one non-NULL max1 row."""
    return [c for c in alive if (scope < 0 or d["scope"][c] == scope) and np.any(d["m1"][d["clip"] == c] != R.NULL)]


_counts_cache = {}


def base_counts(oracle, d, h, tol, low=-1, high=-1):
    """Every clip's count over the frames of h (brute force, no limit), as {clip: count} of the non-zero ones."""
    key = (id(d), h.tobytes(), tol, low, high)
    if key not in _counts_cache:
        got = {}
        if len(h):
            _, qdb, _ = oracle.fingerprint(h)
            rows = R.brute_force(oracle, d["uuids"], d["clip"], d["m1"], d["m2"], list(qdb[:, 0]), list(qdb[:, 1]), 1, tol,
                                 low, high)
            got = {d["uuids"].index(u): n for u, n in rows}
        _counts_cache[key] = got
    return _counts_cache[key]


def verdict(oracle, d, h, total, tol, scope, alive, low=-1, high=-1):
    """The verdict of one channel with samples h of a planned total, from the rule as the header states it."""
    S = len(h)
    complete = S == total
    ffin = S // 256
    cnt = base_counts(oracle, d, h if complete else h[:256 * ffin], tol, low, high)
    remaining = 0 if complete else oracle.frame_count(total) - ffin
    order = sorted(((cnt.get(c, 0), d["uuids"][c]) for c in candidates(d, scope, alive)), reverse=True)
    leader = rival = None
    if order and order[0][0] >= 1:
        leader = order[0]
        rival = order[1] if len(order) > 1 else None
    decided = complete or (leader is not None and (rival is None or leader > (rival[0] + remaining, rival[1])))

    def row(x):
        return None if x is None else (x[1], x[0])
    return {"leader": row(leader), "rival": row(rival), "remaining": remaining, "complete": complete, "decided": decided}


def as_oracle(v):
    """A Live.verdict entry in the oracle's form (clip_id dropped)."""
    def row(x):
        return None if x is None else (x["audio_uuid"], x["match_count"])
    return {"leader": row(v["leader"]), "rival": row(v["rival"]), "remaining": v["remaining"], "complete": v["complete"],
            "decided": v["decided"]}


def raw_verdict(tfp_lib, live, totals, p, scopes=None, mark=77):
    """The C call itself on a live object's handle, into an out array pre-filled with `mark`:
    (return code, the array), so a test sees what a refused call leaves in out."""
    import ctypes as C

    from tiresias_amd._lib import LiveVerdict
    n = live.nchannels
    raw = (LiveVerdict * n)()
    for v in raw:
        v.has_leader = v.remaining = v.decided = mark
    tot = np.ascontiguousarray(totals, np.int64)
    sc = None if scopes is None else np.ascontiguousarray(scopes, np.int32)
    fn = getattr(tfp_lib.lib(), live._PFX + "_verdict")
    rc = fn(live._h, tot.ctypes.data, C.byref(p) if p is not None else None, None if sc is None else sc.ctypes.data, raw)
    return rc, raw


ALIVE = [c for c in range(NCLIPS) if c != REMOVED]

# The 8 calls of the main test: (source, scope, total samples). total % 256 covers 0, 1 and 255, one
# call is a single tick, one fills the live object (MAX_SAMPLES).
MAX_SAMPLES = 12288
CALLS = [
    (("clip", 6, 0), 0, 12288),                 # a clip of its own scope, from its start: total == max_samples, % 256 == 0
    (("clip", 7, 1024), 1, 5121),               # % 256 == 1
    (("clip", TWIN[0], 512), 1, 6399),          # the twins' scope; % 256 == 255
    (("clip", REMOVED, 256), -1, 4000),         # plays the removed clip, over every scope
    (("switch", 2, 12, 4800), -1, 12000),       # clip 2 for 0.6 s, then clip 12
    (("zeros",), 2, 3000),                      # silence: no frame runs its SQL, so there is never a leader
    (("clip", LONE, 768), LONE_SCOPE, 2560),    # a scope with a single clip
    (("clip", 3, 0), 0, 160),                   # a single tick
]


@functools.lru_cache(maxsize=None)
def call_pcm(i):
    src, _, total = CALLS[i]
    if src[0] == "clip":
        x = clip_pcm(src[1])[src[2]:src[2] + total]
    elif src[0] == "switch":
        x = np.concatenate([clip_pcm(src[1])[:src[3]], clip_pcm(src[2])[:total - src[3]]])
    else:
        x = np.zeros(total, np.int16)
    assert len(x) == total
    return x


def lengths(total, tick=T):
    """The samples so far after each push of `tick` samples up to total."""
    return [min(total, (i + 1) * tick) for i in range((total + tick - 1) // tick)]


def oracle_run(oracle, d, i, tol=TOL):
    src, scope, total = CALLS[i]
    x = call_pcm(i)
    return [verdict(oracle, d, x[:S], total, tol, scope, ALIVE) for S in lengths(total)]


def assert_data(oracle):
    """What the tests need of the data, on the CPU oracle alone."""
    d = db(oracle)
    runs = [oracle_run(oracle, d, i) for i in range(len(CALLS))]
    early = [i for i, r in enumerate(runs) if any(v["decided"] and not v["complete"] for v in r)]
    assert early, "no call is decided before it is complete"
    turned = [i for i, r in enumerate(runs)
              if any(v["leader"] and v["leader"][0] != r[-1]["leader"][0] for v in r[:-1] if r[-1]["leader"])]
    assert turned, "no call's mid-call leader differs from its final winner"
    assert any(all(v["leader"] is None for v in r) for r in runs), "every call has a leader at some push"
    return runs
