"""The relaxed flood's three entry points are exported by the built library, declared by the header and bound by the Python layer
(no compute: runs without a GPU)."""
import os
import re

import pytest

from libcimbar_amd import decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cimbar_hip_set_relaxed_flood", "cimbar_hip_get_relaxed_flood", "cimbar_hip_relaxed_flood_stats")


def test_library_exports_the_relaxed_flood_entry_points():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = decoder.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS, name


def test_header_declares_them_and_the_tap_values():
    text = open(os.path.join(ROOT, "include", "cimbar_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"CIMBAR_HIP_TAP_FLOOD_ROUNDS\s*=\s*%d\b" % decoder.TAP_FLOOD_ROUNDS, code)
    assert re.search(r"#define\s+CIMBAR_HIP_RELAXED_FLOOD_SUGGESTED\s+%d\b" % decoder.RELAXED_FLOOD_SUGGESTED, code)
    for method in ("set_relaxed_flood", "get_relaxed_flood", "relaxed_flood_stats"):
        assert callable(getattr(decoder.HipDecoder, method))


def test_null_context_is_refused():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built")
    lib = decoder.load_library()
    assert lib.cimbar_hip_set_relaxed_flood(None, 12, 1) == -1          # CIMBAR_HIP_EINVAL
    assert lib.cimbar_hip_get_relaxed_flood(None, None, None) == -1
    assert lib.cimbar_hip_relaxed_flood_stats(None, None) == -1
