"""The catalog-neighbour entry points (tfp_index_neighbours, tfp_neighbour_stats,
tfp_group_index_neighbours): exported by the library, declared in the header with the reference lines
they stand on, bound in the ctypes mirror; and the argument rules that need no device. No GPU."""
import ctypes as C
import re

NEW_SYMBOLS = ["tfp_index_neighbours", "tfp_neighbour_stats", "tfp_group_index_neighbours"]
TFP_E_ARG = -1


def test_symbols_exported_declared_and_bound(tfp_lib):
    from tiresias_amd import _lib
    syms = _lib.header_symbols()
    lib = tfp_lib.lib()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    for cls in (tfp_lib.Engine, tfp_lib.Group):
        for m in ("index_neighbours", "neighbour_stats"):
            assert callable(getattr(cls, m))


def test_header_cites_the_reference(tfp_lib):
    from tiresias_amd import _lib
    with open(_lib.HEADER) as f:
        src = f.read()
    sec = src[src.index("/* ---- catalog neighbours"):src.index("/* ---- device groups")]
    for cite in ("fp_handler.c:287-374", "fp_handler.c:713-753", "fp_handler.c:367-374", "fp_handler.c:308-314"):
        assert cite in sec, cite
    decls = list(re.finditer(r"^int\s+(tfp_[a-z_]*neighbour[a-z_]*)\(", src, re.M))
    assert sorted(m.group(1) for m in decls) == sorted(NEW_SYMBOLS)
    for m in decls:  # every declaration stands under a comment that names both reference ranges
        above = src[:m.start()]
        comment = above[above.rindex("/*"):]
        assert "fp_handler.c:287-374" in comment and ":713-753" in comment, m.group(1)


def test_argument_rules_that_need_no_device(tfp_lib):
    lib = tfp_lib.lib()
    p = tfp_lib.params(1, 0.001)
    names = (C.c_char_p * 1)(b"a")
    from tiresias_amd import _lib
    out, cnt = (_lib.Candidate * 4)(), (C.c_int32 * 1)(7)
    assert lib.tfp_index_neighbours(None, 1, names, C.byref(p), None, 4, out, None, cnt, None) == TFP_E_ARG
    assert lib.tfp_index_neighbours(None, 0, None, C.byref(p), None, 4, None, None, None, None) == TFP_E_ARG
    assert lib.tfp_group_index_neighbours(None, 1, names, C.byref(p), None, 4, out, None, cnt, None) == TFP_E_ARG
    assert lib.tfp_neighbour_stats(None, None, None, None, None) == TFP_E_ARG
    assert cnt[0] == 7 and out[0].match_count == 0
