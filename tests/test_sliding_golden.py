"""The sliding-search fixture (tests/golden/sliding_cases.json) checked by two independent routes, the
host-only window count, and the sliding entry points' presence in the header and the ctypes binding.
No GPU."""
import os
import subprocess
import sys

import ranked_util as R
import scoped_util as S
import sliding_util as W

NEW_SYMBOLS = ["tfp_sliding_windows", "tfp_search_sliding_batch", "tfp_search_sliding_pcm_batch", "tfp_slide_stats",
               "tfp_group_search_sliding_batch", "tfp_group_search_sliding_pcm_batch"]


def test_generator_check_reproduces_the_fixture():
    """Route 1: peeling the reference's SQL per window (make_golden_sliding.py --check), byte for byte."""
    r = subprocess.run([sys.executable, os.path.join(R.GOLDEN, "make_golden_sliding.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(os.path.join(R.GOLDEN, "sliding_cases.json")) < 200_000


def test_brute_force_over_each_window_equals_peeled_rows(oracle):
    """Route 2: ranked_util.brute_force over each window's frames (a context's clips alone for a scoped
    case). Every window of every case."""
    scen, _ = R.load_cases()
    cases = W.load_sliding()
    W.no_empty_shell(cases)
    seen = set()
    for name, qi, window, hop, ctx, wins in cases:
        s, q = scen[name], scen[name]["queries"][qi]
        F = len(q["q1"])
        assert F >= 12 and q["coefs"] in (1, 2)
        assert window in (1, 4, 16, F) and hop in (1, 3, window, window + 2)
        assert len(wins) == W.nwin(F, window, hop)
        db = S.restrict(s, ctx) if ctx >= 0 else (s["uuids"], s["clip"], s["m1"], s["m2"])
        for w, rows in enumerate(wins):
            a = w * hop
            got = R.brute_force(oracle, *db, q["q1"][a:a + window], q["q2"][a:a + window], q["coefs"], q["tol"], q["low"],
                                q["high"], limit=W.RANKS)
            assert got == rows, (name, qi, window, hop, ctx, w)
        seen.add((q["coefs"], ctx >= 0))
    assert seen == {(1, False), (1, True), (2, False), (2, True)}


def test_sliding_windows_is_the_formula(tfp_lib):
    fn = tfp_lib.lib().tfp_sliding_windows
    for window in (1, 2, 7, 94):
        for hop in (1, 3, window, window + 2, 500):
            for F in (0, 1, window - 1, window, window + 1, window + hop - 1, window + hop, 1875):
                assert fn(F, window, hop) == (W.nwin(F, window, hop) if F > 0 else 0), (F, window, hop)
                assert tfp_lib.sliding_windows(F, window, hop) == fn(F, window, hop)
    assert fn(93, 94, 1) == 0 and fn(94, 94, 1) == 1  # F = window - 1, F = window
    assert fn(10, 4, 11) == 1                        # hop > F: window 0 alone
    assert fn(1875, 94, 1) == 1782 and fn(1875, 94, 8) == 223 and fn(1875, 94, 94) == 19
    for bad in ((0, 4, 1), (-5, 4, 1), (10, 0, 1), (10, -1, 1), (10, 4, 0), (10, 4, -3)):
        assert fn(*bad) == 0, bad
    assert fn(2**40, 1, 1) == 2**40  # 64-bit frame counts


def test_header_and_binding_have_the_sliding_entry_points():
    sys.path.insert(0, os.path.join(R.REPO, "asterisk-tiresias_amd"))
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
    assert _lib.TFP_SLIDE_RUN == 32
    with open(_lib.HEADER) as f:
        assert "#define TFP_SLIDE_RUN 32" in f.read()
