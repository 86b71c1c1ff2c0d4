"""The aligned-search fixture (tests/golden/aligned_cases.json) checked by two independent routes, and
the aligned entry points' presence in the header and the ctypes binding. No GPU."""
import os
import subprocess
import sys

import align_util as A
import ranked_util as R

NEW_SYMBOLS = ["tfp_align_batch", "tfp_search_aligned_batch", "tfp_search_aligned_pcm_batch",
               "tfp_group_search_aligned_batch", "tfp_align_stats"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: the reference's predicate text run by SQLite (make_golden_aligned.py --check), byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_aligned.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_brute_force_equals_the_fixture_and_hit_frames_equal_match_count(oracle):
    """Route 2: a numpy histogram over the oracle's frame boxes reproduces the four integers of every
    pair, and the query frames with any hit in the clip number the ranked fixture's match_count."""
    scen, ranked = R.load_cases()
    aligned = A.load_aligned()
    pairs = tied = negative = coefs2 = 0
    for (name, qi), rows in ranked.items():
        got = aligned.get((name, qi), [])
        assert [u for u, *_ in got] == [u for u, _ in rows[:3]], (name, qi)  # every query, rows 0..2
        s = scen[name]
        q = s["queries"][qi]
        col = {u: c for c, u in enumerate(s["uuids"])}
        for (uuid, *four), (_, match_count) in zip(got, rows):
            m1, m2 = A.clip_rows(s, col[uuid])
            exp, hit_frames, tie = A.brute_force(oracle, m1, m2, q["q1"], q["q2"], q["coefs"], q["tol"], q["low"],
                                                 q["high"], more=True)
            assert tuple(four) == exp, (name, qi, uuid)
            assert hit_frames == match_count, (name, qi, uuid)
            assert 1 <= four[0] <= match_count <= q["frame_count"]
            tied += tie
            negative += four[1] < 0
            coefs2 += q["coefs"] == 2
            pairs += 1
    # the fixture exercises the tie rule, the sign and both predicates
    assert pairs == sum(len(v) for v in aligned.values()) == 1959
    assert tied > 1000 and negative > 1000 and coefs2 > 500, (tied, negative, coefs2)


def test_header_and_binding_have_the_aligned_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
