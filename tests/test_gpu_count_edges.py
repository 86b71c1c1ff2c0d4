"""Plain search at the capacity of every narrow counter, with the form that served each batch asserted
(Engine.search_path_stats, Engine.sweep_stats) and every result compared with the CPU oracle's search
of the same rows (uuid, match_count, frame_count: integers, no tolerance).

  counter                                   limit                      guard
  fp16 per-key counts (build_A_kernel)      exact up to 2048           VoteMeta::ok cleared, batch redone
  packed argmax 1024 * score + column       < 2^24: score <= 16383     max_frames < 16384 (search_core)
  small vote (search_small)                 <= 2048 frames per query   the vote serves the batch
  sweep prefix counts, 4 x 8 bit per word   queries under 256 frames   128-query chunks, 2 x 16 bit
  sweep prefix counts, 2 x 16 bit per word  under 65536 frames         the cells form / row scan
  bin sort place field (kPlaceBits = 18)    chunk x max frames < 2^18  the library sort

Queries are (q1, q2) frames, so nothing is fingerprinted. Every case first asserts on the oracle's
answer alone that the winner's count is the edge value meant: inputs that miss the edge fail the test."""
import os

import numpy as np
import pytest

import ranked_util as R

pytestmark = pytest.mark.gpu

K0 = 20  # first key of the crafted indexes: rows at k * 10^6 + 500, inside key k's box at any tolerance used here
PATHS = ("small", "vote_class", "vote_gemm", "vote_redone", "general", "bins", "library", "redone")


def _engine_with(tfp_lib, env):
    """A fresh engine created with test knobs in the environment (the engine reads them once)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tfp_lib.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Index:
    """Crafted rows (m1 = key * 10^6 + 500, m2 = 0) enrolled so that column c is clip c."""

    def __init__(self, tag, clip_keys):
        self.rows = clip_keys
        self.uuids = ["00000000-%04d-4000-8000-%012d" % (tag, c) for c in range(len(clip_keys))]
        self.foff = np.concatenate([[0], np.cumsum([len(k) for k in clip_keys])]).astype(np.int64)
        self.m1 = (np.concatenate(clip_keys).astype(np.int64) * 1_000_000 + 500).astype(np.int32)
        self.m2 = np.zeros(len(self.m1), np.int32)
        self.clip = np.repeat(np.arange(len(clip_keys)), np.diff(self.foff)).astype(np.int32)
        self.memo = {}

    def enrol(self, eng):
        eng.index_clear()
        eng.index_add_batch(self.uuids, self.foff, self.m1, self.m2)

    def last_with(self, key):
        """The greatest column (uuid) with a row in the key's box."""
        return max(c for c, keys in enumerate(self.rows) if key in keys)

    def expect(self, oracle, q1, coefs, tol):
        """The oracle's (uuid, match_count) or None, memoised: a batch repeats a few distinct queries."""
        key = (coefs, tol, len(q1), q1.tobytes())
        if key not in self.memo:
            found, w, mc, fc = oracle.search(self.m1, self.m2, self.clip, self.uuids, q1, np.zeros(len(q1)), coefs, tol, -1, -1)
            assert fc == len(q1)
            self.memo[key] = (self.uuids[w], mc) if found else None
        return self.memo[key]


def vote_index(nkeys):
    """1,030 clips over nkeys keys: columns 1022 and 1023 are twins with a row in every key's box, column
    1024 lacks the last key, every other clip has one row. A query over all the keys ties the twins,
    column 1023 wins on the tie key alone, and its packed accumulator carries the position field at its
    maximum: 1024 * score + 1023."""
    keys = np.arange(K0, K0 + nkeys)
    rows = [keys if c in (1022, 1023) else keys[:-1] if c == 1024 else keys[c % nkeys:c % nkeys + 1] for c in range(1030)]
    return Index(4000 + nkeys, rows)


def sweep_index():
    """40 clips of one row each over 5 keys: key K0 + j is won by column 35 + j."""
    return Index(5000, [np.array([K0 + c % 5]) for c in range(40)])


def frames_of(counts, seed=0):
    """q1 of a query with counts[key] frames per key, in a fixed shuffled order; trunc(q1) is the key."""
    q1 = np.concatenate([np.full(n, k + 0.25) for k, n in counts.items()] or [np.zeros(0)])
    return np.random.default_rng(seed).permutation(q1)


MISS = np.array([K0 - 5 + 0.25])  # one frame of a key no row has: the query finds nothing (count 0)


def run(eng, oracle, idx, queries, coefs, tol, tfp_lib):
    """The batch through search_batch, every query equal to the oracle's; returns (the oracle's answers,
    the batches each form served)."""
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    q1 = np.concatenate(queries)
    before = {**eng.search_path_stats(), **eng.sweep_stats()}
    res, fcs = eng.search_batch(R.frames_from_q(q1, np.zeros(len(q1))), qoff, tfp_lib.params(coefs, tol))
    now = {**eng.search_path_stats(), **eng.sweep_stats()}
    exp = [idx.expect(oracle, q, coefs, tol) for q in queries]
    for i, q in enumerate(queries):
        got = None if res[i] is None else (res[i]["audio_uuid"], res[i]["match_count"])
        assert got == exp[i], (i, len(q))
        assert fcs[i] == len(q), i
    return exp, {k: now[k] - before[k] for k in PATHS}


def took(delta, **want):
    """The forms and sorts named took exactly these batches, every other one none."""
    assert delta == {**dict.fromkeys(PATHS, 0), **want}, delta


def took_forms(delta, **want):
    """The same over the search forms alone: a coefs = 1 batch on the general path has no max2 windows,
    and which sort its sweep takes is not this file's matter."""
    forms = {k: delta[k] for k in PATHS[:5]}
    assert forms == {**dict.fromkeys(PATHS[:5], 0), **want}, delta


def fillers(keys, n=9):
    """Short queries over the given keys: with them a batch is past the small vote's 8 queries."""
    return [frames_of({int(keys[(i + j) % len(keys)]): 1 + (i + j) % 3 for j in range(1 + i % 4)}, i) for i in range(n)]


def spread(n, keys):
    """n frames over the keys, as evenly as they divide."""
    return {int(k): n // len(keys) + (i < n % len(keys)) for i, k in enumerate(keys)}


# ---- the vote ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gemm_engine(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng = _engine_with(tfp_lib, {"TFP_VOTE_CLASS_MAX": "-1"})  # every vote batch takes the GEMM
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def vote_engine(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    eng = tfp_lib.Engine(0)  # the default knob: up to 10 used keys take the pattern classes
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def indexes():
    return {}


def _enrolled(indexes, eng, make, *args):
    """The crafted index, built once per module and enrolled when the engine holds another."""
    idx = indexes.get((make, args)) or indexes.setdefault((make, args), make(*args))
    if indexes.get(id(eng)) is not idx:
        idx.enrol(eng)
        indexes[id(eng)] = idx
    return idx


# 12 keys: Kp = 16, A and B in registers; 40 keys: Kp = 48, the LDS-staged tiles; 140 keys: Kp = 144, the
# streamed tiles. Each keeps its own accumulators and ends in vote_reduce_rows.
@pytest.mark.parametrize("nkeys", [12, 40, 140])
@pytest.mark.parametrize("n", [16383, 16384])
def test_packed_accumulator_at_2_pow_24(gemm_engine, oracle, tfp_lib, indexes, nkeys, n):
    """A score of 16383 on column 1023 of a chunk: the fp32 accumulator is exactly 2^24 - 1, the last
    value before integers stop being exact. One frame more and the vote must not be tried at all."""
    idx = _enrolled(indexes, gemm_engine, vote_index, nkeys)
    keys = np.arange(K0, K0 + nkeys)
    counts = spread(n, keys)
    assert max(counts.values()) <= 2048 and sum(counts.values()) == n
    queries = [frames_of(counts)] + fillers(keys)
    exp, d = run(gemm_engine, oracle, idx, queries, 1, 0.001, tfp_lib)
    assert exp[0] == (idx.uuids[1023], n)  # the edge, by the oracle alone: the twins tie, the later column wins
    assert 1024 * 16383 + 1023 == 2**24 - 1
    if n == 16383:
        took(d, vote_gemm=1)
    else:
        took_forms(d, general=1)


@pytest.mark.parametrize("form", ["gemm", "class"])
@pytest.mark.parametrize("n", [2048, 2049])
def test_fp16_count_at_2048(gemm_engine, vote_engine, oracle, tfp_lib, indexes, form, n):
    """One key with exactly 2048 frames in a query is the last count fp16 holds exactly: the vote stands.
    With 2049 (fp16 would round it to 2048) build_A clears VoteMeta::ok and the batch is redone on the
    general path. Query 0 has n frames of one key and nothing else, so its count is n itself; query 1
    adds 3 frames of every other used key, which the twins collect."""
    eng = gemm_engine if form == "gemm" else vote_engine
    idx = _enrolled(indexes, eng, vote_index, 12)
    keys = np.arange(K0, K0 + 12)[0 if form == "gemm" else 2:]  # the class form: at most 10 used keys
    big = K0 + 3
    mixed = {int(k): n if k == big else 3 for k in keys}
    queries = [frames_of({big: n}), frames_of(mixed)] + fillers(keys)
    exp, d = run(eng, oracle, idx, queries, 1, 0.001, tfp_lib)
    assert idx.last_with(big) == 1024 and K0 + 11 in keys  # (column 1024 lacks key K0 + 11, which query 1 has)
    assert exp[0] == (idx.uuids[1024], n)
    assert exp[1] == (idx.uuids[1023], n + 3 * (len(keys) - 1))
    if n == 2048:
        took(d, **{"vote_gemm" if form == "gemm" else "vote_class": 1})
    else:
        took_forms(d, vote_redone=1, general=1)


@pytest.mark.parametrize("n", [2048, 2049])
def test_small_vote_at_2048_frames(vote_engine, oracle, tfp_lib, indexes, n):
    """8 queries, the longest of 2048 frames: the small vote. One frame more and the vote serves the
    batch, with a per-key count of exactly 2048 in it."""
    idx = _enrolled(indexes, vote_engine, vote_index, 12)
    keys = np.arange(K0, K0 + 12)
    long_q = frames_of({K0 + 3: 2048} if n == 2048 else {K0 + 3: 2048, K0 + 11: 1})
    queries = [long_q] + fillers(keys, 7)
    assert len(queries) == 8 and max(len(q) for q in queries) == n
    exp, d = run(vote_engine, oracle, idx, queries, 1, 0.001, tfp_lib)
    assert exp[0] == ((idx.uuids[1024], 2048) if n == 2048 else (idx.uuids[1023], 2049))
    if n == 2048:
        took(d, small=1)
    else:
        assert d["vote_class"] + d["vote_gemm"] == 1  # (by the batch's used keys)
        took(d, vote_class=d["vote_class"], vote_gemm=d["vote_gemm"])


# ---- the sweep (coefs = 2) ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep_engines(tfp_lib):
    if tfp_lib.device_count() < 1:
        pytest.skip("no GPU visible")
    engs = {"sweep": _engine_with(tfp_lib, {"TFP_WIDE_MIN_TOL": "0"}),
            "ch128": _engine_with(tfp_lib, {"TFP_WIDE_MIN_TOL": "0", "TFP_WIDE_CH128": "1"}),
            "cells": _engine_with(tfp_lib, {"TFP_WIDE_MIN_TOL": "1e9"})}
    yield engs
    for e in engs.values():
        e.close()


def _byte_lanes(full=255):
    """260 queries (two 256-query chunks, the second partial): the four queries of lane l hold counts
    full, 0, full, 1 rotated by l, so every byte of a lane word is at `full` beside neighbours that must
    not take a carry; the keys differ by lane. Lane 63's last byte and the batch's last query are full."""
    queries = []
    for i in range(260):
        lane, b = divmod(i % 256, 4)
        kind = (full, 0, full, 1)[(b - lane) % 4] if i < 256 else (1, 0, 1, full)[i - 256]
        key = K0 + lane % 5
        queries.append(MISS if kind == 0 else frames_of({key: kind}))
    assert len(queries[255]) == full and len(queries[259]) == full
    for lane in (0, 1, 2, 3, 63):
        assert sorted(len(q) for q in queries[4 * lane:4 * lane + 4]) == [1, 1, full, full]
    assert {b for i in range(256) if len(queries[i]) == full for b in [i % 4]} == {0, 1, 2, 3}
    return queries


@pytest.mark.parametrize("tol", [0.001, 0.45])
def test_sweep_byte_counts_at_255(sweep_engines, oracle, tfp_lib, indexes, tol):
    """Every query under 256 frames: 256-query chunks, four 8-bit prefix counts per lane word."""
    eng = sweep_engines["sweep"]
    idx = _enrolled(indexes, eng, sweep_index)
    queries = _byte_lanes()
    assert max(len(q) for q in queries) == 255
    exp, d = run(eng, oracle, idx, queries, 2, tol, tfp_lib)
    assert exp[0] == (idx.uuids[35], 255) and exp[1] is None and exp[3] == (idx.uuids[35], 1)
    assert exp[255] == (idx.uuids[35 + 63 % 5], 255) and exp[259] == (idx.uuids[35], 255)
    took(d, general=1, bins=1)
    # the same batch in 128-query chunks (two 16-bit counts per word)
    eng = sweep_engines["ch128"]
    idx = _enrolled(indexes, eng, sweep_index)
    _, d = run(eng, oracle, idx, queries, 2, tol, tfp_lib)
    took(d, general=1, bins=1)


@pytest.mark.parametrize("tol", [0.001, 0.45])
def test_sweep_one_query_of_256_frames(sweep_engines, oracle, tfp_lib, indexes, tol):
    """One query lengthened to 256 frames: a byte could not hold its count, the batch takes 128-query
    chunks, and every other query's result is what it was."""
    eng = sweep_engines["sweep"]
    idx = _enrolled(indexes, eng, sweep_index)
    queries = _byte_lanes()
    queries[255] = frames_of({K0 + 63 % 5: 256})
    assert max(len(q) for q in queries) == 256
    exp, d = run(eng, oracle, idx, queries, 2, tol, tfp_lib)
    assert exp[255] == (idx.uuids[35 + 63 % 5], 256) and exp[254] == (idx.uuids[35 + 63 % 5], 1)
    took(d, general=1, bins=1)


def _halfword_pairs(full):
    """Queries 2l and 2l + 1 share a lane word: (full, 0), (0, full), (full, full), (full, 1)."""
    one = frames_of({K0 + 1: 1})
    a, b = frames_of({K0: full}), frames_of({K0 + 2: full})
    return [a, MISS, MISS, b, a, b, b, one]


@pytest.mark.parametrize("tol", [0.001, 0.45])
def test_sweep_halfword_counts_at_65535(sweep_engines, oracle, tfp_lib, indexes, tol):
    """Queries of 65535 frames: the 16-bit prefix counts at their maximum beside a neighbour at 0, at 1
    and at 65535. 128 * 65535 >= 2^18, so the library sort orders the frames."""
    eng = sweep_engines["sweep"]
    idx = _enrolled(indexes, eng, sweep_index)
    queries = _halfword_pairs(65535)
    exp, d = run(eng, oracle, idx, queries, 2, tol, tfp_lib)
    assert exp == [(idx.uuids[35], 65535), None, None, (idx.uuids[37], 65535), (idx.uuids[35], 65535),
                   (idx.uuids[37], 65535), (idx.uuids[37], 65535), (idx.uuids[36], 1)]
    took(d, general=1, library=1)


def test_sweep_ineligible_at_65536_frames(sweep_engines, oracle, tfp_lib, indexes):
    """One query of 65536 frames: no 16-bit count holds it, the sweep declines the batch and the cells
    form / row scan serves it with the same results."""
    eng = sweep_engines["sweep"]
    idx = _enrolled(indexes, eng, sweep_index)
    queries = _halfword_pairs(65535)
    queries[0] = frames_of({K0: 65536})
    exp, d = run(eng, oracle, idx, queries, 2, 0.001, tfp_lib)
    assert exp[0] == (idx.uuids[35], 65536) and exp[1] is None and exp[7] == (idx.uuids[36], 1)
    took(d, general=1)


@pytest.mark.parametrize("n", [2047, 2048])
def test_bin_sort_place_field_edge(sweep_engines, oracle, tfp_lib, indexes, n):
    """128 queries (one chunk) of 2047 frames of one key: 262,016 frames in one bin, the greatest place
    an 18-bit field holds with room to spare for none; the bin sort stands. One query at 2048 frames
    and 128 * 2048 = 2^18: the library sort."""
    eng = sweep_engines["sweep"]
    idx = _enrolled(indexes, eng, sweep_index)
    q = frames_of({K0 + 4: 2047})
    queries = [q] * 127 + [frames_of({K0 + 4: n})]
    assert 128 * 2047 < 2**18 <= 128 * 2048
    exp, d = run(eng, oracle, idx, queries, 2, 0.001, tfp_lib)
    assert exp[0] == (idx.uuids[39], 2047) and exp[127] == (idx.uuids[39], n)
    took(d, general=1, **{"bins" if n == 2047 else "library": 1})


@pytest.mark.parametrize("path", ["sweep", "cells"])
@pytest.mark.parametrize("n", [2049, 16384])
def test_vote_fallback_takes_the_general_form(sweep_engines, oracle, tfp_lib, indexes, path, n):
    """coefs = 1 past the vote's counters, through both general forms: 2049 frames of one key (the vote
    runs and is redone) and 16384 frames (the vote is not tried)."""
    eng = sweep_engines[path]
    idx = _enrolled(indexes, eng, sweep_index)
    keys = np.arange(K0, K0 + 5)
    queries = [frames_of({K0 + 2: n})] + fillers(keys)
    exp, d = run(eng, oracle, idx, queries, 1, 0.001, tfp_lib)
    assert exp[0] == (idx.uuids[37], n)
    took_forms(d, general=1, **({"vote_redone": 1} if n == 2049 else {}))
    assert (d["bins"] + d["library"] > 0) == (path == "sweep")  # the form the engine's knob selects
