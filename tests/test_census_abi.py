"""The census entry points in the header, the binding and the library, and the host-only
tfp_census_at_least on hand rows. No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import ranked_util as R

NEW_SYMBOLS = ["tfp_census_batch", "tfp_census_pcm_batch", "tfp_census_stats", "tfp_census_at_least",
               "tfp_group_census_batch", "tfp_group_census_pcm_batch"]


def test_header_binding_and_library_have_the_census_entry_points(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
    out = subprocess.run(["nm", "-D", "--defined-only", tfp_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
    with open(os.path.join(R.REPO, "shim", "fp_handler_tfp.h")) as f:
        assert "fp_search_fingerprint_census(" in f.read()
    assert hasattr(tfp_lib.Engine, "census_batch") and hasattr(tfp_lib.Group, "census_pcm_batch")
    assert hasattr(tfp_lib.FpHandler, "fp_search_fingerprint_census")


def test_census_at_least_on_hand_rows(tfp_lib):
    at_least = tfp_lib.lib().tfp_census_at_least

    def f(row, count):
        a = np.asarray(row, np.int32)
        got = at_least(a.ctypes.data, len(a), count)
        assert got == tfp_lib.census_at_least(row, count)
        return got

    row = [7, 0, 3, 0, 2, 1]  # 7 clips without a hit, 3 at count 2, 2 at 4, 1 at 5
    assert [f(row, c) for c in range(1, 8)] == [6, 6, 3, 3, 1, 0, 0]
    assert f(row, 0) == f(row, -1) == f(row, -(2**31)) == 13  # bin 0 only for count <= 0
    assert f(row, 2**31 - 1) == 0
    assert f([5], 0) == 5 and f([5], 1) == 0  # a query without frames: bin 0 alone
    assert f([0, 0, 0], 0) == 0
    assert at_least(None, 0, 0) == 0 and at_least(None, 4, 1) == 0
    big = [0, 2**31 - 1, 2**31 - 1, 2**31 - 1]  # the sum is taken in 64 bits
    assert f(big, 1) == 3 * (2**31 - 1)
    assert at_least.restype is C.c_int64 and sys.maxsize > 2**32
