"""Shared by the tests of live objects with an input rate (tfp_live_create_rate, tfp_group_live_create_rate):
the settled count restated, the exact check of a rate object's history through its kept frames, and the twin
run (a rate object against a plain object that is pushed each step's newly settled samples)."""
import numpy as np

import live_util as L
import resample_util as RU

SEED16 = 0x16AE


def lag_of(rate_in, rate_out):
    return RU.plan(rate_in, rate_out)[3]  # k_hi


def settled(s_in, rate_in, rate_out):
    """N(S_in) = resample_count(S_in - k_hi), 0 while S_in <= k_hi."""
    L_, M, _, k_hi = RU.plan(rate_in, rate_out)
    return RU.count(s_in - k_hi, L_, M)


def n_in_for(s_in, new, rate_in, rate_out):
    """The fewest further input samples that settle exactly `new` more outputs (None where no count does)."""
    base = settled(s_in, rate_in, rate_out)
    n = 0
    while settled(s_in + n, rate_in, rate_out) < base + new:
        n += 1
    return n if settled(s_in + n, rate_in, rate_out) == base + new else None


class Call:
    """The input each channel has been pushed so far, and the checks of the object against it."""

    def __init__(self, tfp, owner, lv, rate_in, rate_out, src):
        self.tfp, self.owner, self.lv, self.ri, self.ro = tfp, owner, lv, rate_in, rate_out
        self.src = [np.ascontiguousarray(x, np.int16) for x in src]
        self.at = [0] * len(src)  # input samples taken, per channel

    def tick(self, want):
        """The next want[c] samples of every channel's source as a tick (fewer where a source ends)."""
        n = [min(int(w), len(x) - a) for w, x, a in zip(want, self.src, self.at)]
        blk = np.zeros((len(n), max(max(n), 1)), np.int16)
        for c, k in enumerate(n):
            blk[c, :k] = self.src[c][self.at[c]:self.at[c] + k]
        return blk, n

    def took(self, n):
        self.at = [a + k for a, k in zip(self.at, n)]

    def push(self, want, p=None, **kw):
        blk, n = self.tick(want)
        res = self.lv.push(blk, p, nsamples=n, **kw)
        self.took(n)
        return res

    def expected(self, c, flushed=False):
        """The channel's history by the definition: the first N(S_in) samples of resample_pcm of its input so
        far (flushed: all of them)."""
        y = self.tfp.resample_pcm(self.src[c][:self.at[c]], self.ri, self.ro)
        return y if flushed else y[:settled(self.at[c], self.ri, self.ro)]

    def check(self, where=None, flushed=False):
        """samples, input_samples and the kept frames of every channel, bit for bit."""
        exp = [self.expected(c, flushed) for c in range(len(self.src))]
        off = np.concatenate([[0], np.cumsum([len(y) for y in exp])])
        fr = self.owner.fingerprint_batch(np.concatenate(exp), off, self.ro) if off[-1] else np.zeros(0)
        foff = np.concatenate([[0], np.cumsum([self.tfp.frame_count(len(y)) for y in exp])])
        for c, y in enumerate(exp):
            assert self.lv.input_samples(c) == self.at[c], (where, c)
            assert self.lv.samples(c) == len(y), (where, c, self.at[c], self.lv.samples(c), len(y))
            got = self.lv.frames(c, 0)
            if not len(y):
                assert len(got) == 0, (where, c)
                continue
            want = fr[foff[c]:foff[c + 1]].copy()
            want["frame_idx"] -= want["frame_idx"][0] - got["frame_idx"][0] if len(got) else 0
            try:
                RU.bits_equal(got, want)
            except AssertionError as e:
                raise AssertionError((where, c, self.at[c], len(y), e.args)) from None


def sources16(tfp):
    """16 kHz sources, one per clip of live_util's DB (the twin clips share theirs), twice a clip's length."""
    return {c: tfp.synth_pcm(SEED16, [c], 2 * L.clip_len(c))[0] for c in range(L.NCLIPS) if c != L.TWIN[1]}


def build_db16(tfp, owner):
    """live_util.build_db with every enrolled clip the resample_pcm (16000 -> 8000) of a 16 kHz source. Returns
    (db, sources)."""
    src = sources16(tfp)
    old = L.clip_pcm
    L.clip_pcm = lambda t, c: t.resample_pcm(src[L.TWIN[0] if c == L.TWIN[1] else c], 16000, 8000)
    try:
        db = L.build_db(tfp, owner)
    finally:
        L.clip_pcm = old
    return db, src


TWIN_CALLS = ((7, 0), (L.TWIN[0], 512), (12, 1024), (20, 2 * 512))  # (clip, input offset: a multiple of 256 M)
TWIN_SCOPES = [7 % 3, -1, 12 % 3, -1]
TWIN_IN = 14 * 512 + 77  # input samples per call: 14 frames and a tail at 8 kHz
WINDOW, K, GAP, HITS = 6, 3, 3, 4


def strip(x):
    """A result without its clip ids (a group's are shards)."""
    if isinstance(x, dict):
        return {k: strip(v) for k, v in x.items() if k != "clip_id"}
    if isinstance(x, (list, tuple)):
        return [strip(v) for v in x]
    return x


def run_twin(tfp, owner, make_live, src16, p):
    """A rate object (16000 -> 8000) against a plain object at 8 kHz that is pushed each step's newly settled
    samples (resample_pcm on the host): equal push rows and frame counts every step, equal window,
    window_aligned and occurrences every third step and at the end, an equal verdict after finish. Returns
    everything the rate object returned."""
    nch = len(TWIN_CALLS)
    x = [src16[c][o:o + TWIN_IN] for c, o in TWIN_CALLS]
    y = [tfp.resample_pcm(v, 16000, 8000) for v in x]  # the settled samples are a prefix of it
    cap = max(len(v) for v in y)
    a, b = make_live(owner, nch, cap, 16000), make_live(owner, nch, cap, None)
    call = Call(tfp, owner, a, 16000, 8000, x)
    out = []
    ticks = [1, 3, 96, 97, 320] + [640, 333] * 20
    step = 0
    while min(call.at) < TWIN_IN:
        t = ticks[step]
        want = [0 if (c == 0 and step % 4 == 3) else t + 5 * c for c in range(nch)]
        old = [settled(s, 16000, 8000) for s in call.at]
        rows = call.push(want, p, scopes=TWIN_SCOPES, k=K)
        new = [settled(s, 16000, 8000) for s in call.at]
        blk = np.zeros((nch, max(max(n - o for n, o in zip(new, old)), 1)), np.int16)
        for c in range(nch):
            blk[c, :new[c] - old[c]] = y[c][old[c]:new[c]]
        twin = b.push(blk, p, scopes=TWIN_SCOPES, k=K, nsamples=[n - o for n, o in zip(new, old)])
        assert rows == twin, (step, rows, twin)
        assert [a.samples(c) for c in range(nch)] == new == [b.samples(c) for c in range(nch)], step
        out.append(rows)
        if step % 3 == 2:
            out.append(_same_queries(a, b, p, step))
        step += 1
    out.append(_same_queries(a, b, p, "end"))
    a.finish()
    assert [a.samples(c) for c in range(nch)] == [len(v) for v in y]
    rest = np.zeros((nch, max(len(v) for v in y)), np.int16)
    ns = [len(y[c]) - b.samples(c) for c in range(nch)]
    for c in range(nch):
        rest[c, :ns[c]] = y[c][len(y[c]) - ns[c]:]
    b.push(rest, nsamples=ns)
    out.append(_same_queries(a, b, p, "finished"))
    total = [len(v) for v in y]
    if p.coefs == 1:
        va, vb = a.verdict(total, p, TWIN_SCOPES), b.verdict(total, p, TWIN_SCOPES)
        assert va == vb and all(v["complete"] for v in va), (va, vb)
        out.append(va)
    else:  # the counts a verdict reads are coefs = 1's: both objects refuse alike
        for lv in (a, b):
            try:
                lv.verdict(total, p, TWIN_SCOPES)
                raise AssertionError("a coefs = 2 verdict")
            except tfp.TfpError as e:
                assert e.code == -1
    a.close()
    b.close()
    return out


def _same_queries(a, b, p, where):
    wa, wb = a.window(p, TWIN_SCOPES, K, WINDOW), b.window(p, TWIN_SCOPES, K, WINDOW)
    assert wa == wb, (where, wa, wb)
    la, lb = a.window_aligned(p, TWIN_SCOPES, K, WINDOW), b.window_aligned(p, TWIN_SCOPES, K, WINDOW)
    assert la == lb, (where, la, lb)
    oa = a.occurrences(p, TWIN_SCOPES, K, WINDOW, GAP, HITS)
    ob = b.occurrences(p, TWIN_SCOPES, K, WINDOW, GAP, HITS)
    assert oa == ob, (where, oa, ob)
    return [wa, la, oa]


def assert_not_empty(out):
    """The twin run saw rows on some channel and listed an occurrence."""
    pushes = [r for r in out if isinstance(r, tuple)]
    assert any(rows for r in pushes for rows in r[0]), "no push returned a row"
    queries = [r for r in out if isinstance(r, list) and len(r) == 3 and isinstance(r[2], tuple)]
    assert any(occ for q in queries for occ in q[2][0]), "no occurrence was listed"
