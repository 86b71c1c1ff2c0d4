"""The sliding-aligned-search fixture (tests/golden/sliding_aligned_cases.json) checked by two independent
routes and against becoming an empty shell, and the new entry points' presence in the header and the
ctypes binding. No GPU."""
import os
import subprocess
import sys

import align_util as A
import ranked_util as R
import slide_align_util as SA
import sliding_util as W

NEW_SYMBOLS = ["tfp_align_sliding_batch", "tfp_search_sliding_aligned_batch", "tfp_search_sliding_aligned_pcm_batch",
               "tfp_group_search_sliding_aligned_batch", "tfp_slide_align_stats"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: the reference's predicate text run by SQLite per window frame, byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_sliding_aligned.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(os.path.join(R.GOLDEN, "sliding_aligned_cases.json")) < 200_000


def test_brute_force_equals_the_fixture_for_every_entry(oracle):
    """Route 2: align_util.brute_force over each window's frames and the row's clip's rows."""
    scen, _ = R.load_cases()
    cases = SA.load_sliding_aligned()
    committed = [c for c in cases if not c[6]]
    assert len(committed) == 48 and sum(len(c[5]) for c in committed) == 659  # every window of every sliding case
    entries = 0
    for name, qi, window, hop, ctx, wins, _added in cases:
        s, q = scen[name], scen[name]["queries"][qi]
        col = {u: c for c, u in enumerate(s["uuids"])}
        assert len(wins) == W.nwin(len(q["q1"]), window, hop)
        for w, rows in enumerate(wins):
            a = w * hop
            for uuid, match_count, *four in rows:
                m1, m2 = A.clip_rows(s, col[uuid])
                exp, hit_frames, _ = A.brute_force(oracle, m1, m2, q["q1"][a:a + window], q["q2"][a:a + window], q["coefs"],
                                                   q["tol"], q["low"], q["high"], more=True)
                assert tuple(four) == exp, (name, qi, window, hop, w, uuid)
                assert hit_frames == match_count and 1 <= four[0] <= match_count <= window
                entries += 1
    assert entries > 900


def test_the_fixture_is_no_empty_shell():
    scen, _ = R.load_cases()
    cases = SA.load_sliding_aligned()
    rows = [r for c in cases for win in c[5] for r in win]
    assert 3 * sum(r[2] < r[1] for r in rows) >= len(rows) > 0  # the hits that line up are fewer than the hits
    joined = 0
    for _name, _qi, _window, hop, _ctx, wins, _added in cases:  # a clip keeps offset - w * hop over two consecutive windows
        for w in range(1, len(wins)):
            prev = {r[0]: r[3] - (w - 1) * hop for r in wins[w - 1]}
            if any(prev.get(r[0]) == r[3] - w * hop for r in wins[w]):
                joined += 1
                break
    assert joined >= 1
    assert {scen[c[0]]["queries"][c[1]]["coefs"] for c in cases} == {1, 2}
    assert {c[4] < 0 for c in cases} == {True, False}  # unscoped and scoped


def test_header_and_binding_have_the_new_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
