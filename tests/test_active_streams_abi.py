"""The per-call active-stream mask at the ABI surface (no GPU needed): both entry points are declared in
include/mi_airband.h, exported by the library, listed by the binding and wrapped on the handle class."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi_demod_set_active_streams", "mi_demod_get_active_streams")


def test_mask_entries_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    lib = pkg.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/mi_airband.h"
        assert hasattr(lib, s), f"{s} is not exported by libmi_airband.so"
        assert s in pkg.ABI_SYMBOLS
    assert re.search(r"int\s+mi_demod_set_active_streams\s*\(\s*mi_demod\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*active\s*\)", header)
    assert re.search(r"int\s+mi_demod_get_active_streams\s*\(\s*const\s+mi_demod\s*\*\s*h\s*,\s*uint8_t\s*\*\s*active\s*\)", header)


def test_binding_wraps_the_mask(pkg):
    assert callable(getattr(pkg.Demod, "set_active_streams", None))
    assert callable(getattr(pkg.Demod, "get_active_streams", None))


def test_null_handle_is_an_error_not_a_crash(pkg):
    lib = pkg.lib()
    assert lib.mi_demod_set_active_streams(None, None) == pkg.MI_ERR_INVALID
    assert lib.mi_demod_get_active_streams(None, None) == pkg.MI_ERR_INVALID
