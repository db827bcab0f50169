"""The deskew warp's yardstick on the cases of tests/warp_cases.py: the oracle's co_deskew against the reference build's Deskewer (ref_deskew,
bit-exact) on every case the reference can be asked, and the coverage conditions that keep every case on the path it is in the table for.
The device is held to the same oracle frames in tests/test_gpu_warp_cases.py."""
import ctypes

import numpy as np
import pytest

from oracle import pyref
from oracle.pyref import P
from tests import warp_cases as WC

TABLE = WC.table()


def test_the_table_holds_what_it_promises():
    names = [c.name for c in TABLE]
    assert len(set(names)) == len(names)
    have = {(c.w, c.h, c.fmt, c.quad) for c in TABLE}
    assert WC.BASE == (1920, 1080) and WC.ODD8[0] % 8 == 2 and WC.ODD8[1] % 4 == 2
    for (w, h) in (WC.BASE, WC.ODD8):               # every quad class in every format at 1920x1080 and at a width that is no multiple of 8
        for fmt in WC.FORMATS:
            for q in WC.QUADS:
                assert (w, h, fmt, q) in have
    sizes = {(c.w, c.h) for c in TABLE}
    assert {w % 8 for (w, h) in sizes if w % 2 == 0 and h % 2 == 0 and w > 64} >= {0, 2, 4, 6}
    assert sizes >= set(WC.TINY) | {(1283, 977)}
    for (w, h) in sizes:                            # every size with at least the inscribed and the overhanging quad in every format it can hold
        for fmt in WC.formats_of(w, h):
            assert (w, h, fmt, "inscribed") in have and (w, h, fmt, "overhang") in have
    assert all(c.fmt in (3, 4) for c in TABLE if c.w % 2 or c.h % 2)
    # the classes the reference cannot be asked are exactly those whose corners it would truncate or overflow
    for c in TABLE:
        assert WC.integer_corners(c) == (c.quad not in WC.REF_NO_ANSWER), c.name


@pytest.mark.parametrize("fmt", WC.FORMATS)
def test_every_case_covers_its_path(fmt):
    """the coverage conditions, on the oracle's output: an overhanging case is black along its four edges and not at the centre, a far corner
    leaves 5..95 % black, inscribed / mirrored / rotated cases have no black row, singular quads give a constant frame of source pixel (0, 0),
    the identity quad copies the capture, non-finite corners give black"""
    seen = set()
    for cases in WC.batches([c for c in TABLE if c.fmt == fmt]).values():
        O = pyref.oracle_lib()
        for k, c in enumerate(cases):
            if c.quad not in WC.COVER:
                continue
            rgb = WC.rgb_view(O, WC.capture(c, k), c.w, c.h, c.fmt)
            WC.check_coverage(c, WC.oracle_frame(O, rgb, c.corners), rgb)
            seen.add(WC.COVER[c.quad])
    assert seen == set(WC.COVER.values())


def pin(ref, cases, mode=68):
    """co_deskew == ref_deskew for the cases the reference can be asked; the RGB view of each capture (the conversions are pinned in
    tests/test_capture_formats.py)"""
    O = pyref.oracle_lib(mode)
    iw, ih = WC.frame_size(mode)
    asked = set()
    for batch in WC.batches(cases).values():
        for k, c in enumerate(batch):
            if c.quad in WC.REF_NO_ANSWER:
                continue
            rgb = np.ascontiguousarray(WC.rgb_view(O, WC.capture(c, k), c.w, c.h, c.fmt))
            want = np.zeros((ih, iw, 3), np.uint8)
            assert ref.ref_deskew(P(rgb), c.w, c.h, c.corners.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), P(want)) == ih
            got = WC.oracle_frame(O, rgb, c.corners, mode)
            assert (got == want).all(), f"{c.name}: {(got != want).sum()} bytes differ"
            if mode != 68:          # (mode 68's conditions: test_every_case_covers_its_path)
                WC.check_coverage(c, got, rgb)
            asked.add(c.quad)
    return asked


def test_oracle_deskew_equals_the_reference_on_hostile_quads(ref):
    """every quad class the reference can be asked, at every size of the table (RGB captures), and in the 4:2:0 formats at the two sizes that
    carry every class"""
    cases = [c for c in TABLE if c.fmt == 3 or (c.fmt == 12 and (c.w, c.h) == WC.ODD8 and c.quad in WC.MODE_QUADS)]
    assert pin(ref, cases) == set(WC.QUADS) - set(WC.REF_NO_ANSWER)


@pytest.mark.parametrize("mode", [67, 66])
def test_oracle_deskew_equals_the_reference_in_other_modes(ref, mode):
    """1024x720 and 736x637 frames: the inscribed, overhanging and mirrored quads (and the others of the modes' table) under Config::update(mode)"""
    cases = [c for c in WC.mode_table(mode) if c.fmt == 3]
    with pyref.ref_mode(mode):
        assert pin(ref, cases, mode) >= {"inscribed", "overhang", "mirrored"}
