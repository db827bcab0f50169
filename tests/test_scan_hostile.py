"""CPU: the oracle's anchor search and extract (co_scan_anchors / co_extract) against the reference build's Scanner::scan / Extractor::extract on the
hostile captures of tests/scan_hostile_cases.py -- rotated, mirrored, with decoys, filling the device's lists, odd shapes, anchors at the border,
quads at the is_granular_scale boundary. This is what entitles tests/test_gpu_scan_hostile.py to use the oracle as its yardstick on them. It
also asserts that the families do what they are for, by the oracle's counters (co_scan_debug_*)."""
import numpy as np
import pytest

from libcimbar_amd import framegen, geometry
from oracle import pyref
from oracle.pyref import P
from tests import scan_hostile_cases as C

from tests.scan_hostile_cases import BR_ROWS, CANDIDATES, CONFIRM_CHANGES, EQUAL_SIZES, OUTSIDE, PRIMARY_HITS, ROW_HITS, ROWS, measure


def unstable_sort(m):
    """std::sort on more than 16 candidates with equal sizes among them: libstdc++'s introsort is not stable there"""
    return m["cnt"][CANDIDATES] > 16 and m["cnt"][EQUAL_SIZES] == 1


def compare_with_reference(ref, cam, m, tag, frame_shape=(1024, 1024, 3)):
    h, w = cam.shape[:2]
    a = np.zeros(16, np.int32)
    n = ref.ref_scan_anchors(P(cam), w, h, P(a))
    assert n == m["found"], f"{tag}: reference found {n}, oracle {m['found']}"
    assert (a[:4 * min(n, 4)].reshape(-1, 4) == m["anchors"]).all(), tag
    out = np.zeros(frame_shape, np.uint8)
    rc = ref.ref_extract(P(cam), w, h, P(out))
    assert rc == m["status"], f"{tag}: reference status {rc}, oracle {m['status']}"
    if rc:
        assert (out == m["frame"]).all(), tag


@pytest.fixture(scope="module")
def measured(synth, oracle):
    return C.measure_families(synth, oracle)


@pytest.mark.parametrize("family", ["orientation", "decoys", "shapes"])
def test_oracle_equals_reference(ref, measured, family):
    for name, cam, m in measured[family]:
        assert not unstable_sort(m), f"{name}: only `pressure` cases may meet the unstable sort"
        compare_with_reference(ref, cam, m, name)


def test_oracle_equals_reference_pressure(ref, measured):
    """... except where std::sort's order is not defined (more than 16 candidates, equal sizes among them): at most a quarter of the family"""
    skipped = 0
    for name, cam, m in measured["pressure"]:
        if unstable_sort(m):
            skipped += 1
            continue
        compare_with_reference(ref, cam, m, name)
    assert 4 * skipped <= len(measured["pressure"]), skipped


def test_oracle_equals_reference_edges(ref, measured):
    """... for the cases where no confirm scan tests a pixel outside the image (the reference reads out of bounds there, the port reads "inactive"):
    decided per case by the oracle's counter of such tests. At least half of the family is compared."""
    compared = 0
    for name, cam, m in measured["edges"]:
        assert not unstable_sort(m), name
        if m["cnt"][OUTSIDE]:
            continue
        compare_with_reference(ref, cam, m, name)
        compared += 1
    assert 2 * compared >= len(measured["edges"]), compared


@pytest.mark.parametrize("mode", [68, 67, 66])
def test_scale_family_both_verdicts_and_reference(ref, mode):
    """is_granular_scale at its boundary: the anchor-centre distances step through IMG_W - 2 .. IMG_W + 2 and IMG_H - 2 .. IMG_H + 2, both
    verdicts (1 SUCCESS, 2 NEEDS_SHARPEN) occur, and oracle == reference in this mode"""
    geo = geometry.for_mode(mode)
    O = pyref.oracle_lib(mode)
    seen, dxs, dys, one_axis = set(), set(), set(), set()
    with pyref.ref_mode(mode) as R:
        for name, cam in C.scale(framegen.FrameSynth("cpu", mode), mode):
            m = measure(O, cam, geo.FRAME_SHAPE)
            assert m["found"] == 4 and not unstable_sort(m), name
            compare_with_reference(R, cam, m, name, geo.FRAME_SHAPE)
            c = m["corners"]
            dx, dy = c[2] - c[0], c[5] - c[1]
            assert m["status"] == (1 if dx > geo.IMG_W and dy > geo.IMG_H and c[6] - c[4] > geo.IMG_W and c[7] - c[3] > geo.IMG_H else 2), name
            seen.add(m["status"]); dxs.add(int(dx) - geo.IMG_W); dys.add(int(dy) - geo.IMG_H)
            if dx == geo.IMG_W and dy > geo.IMG_H:
                one_axis.add("x")
            if dy == geo.IMG_H and dx > geo.IMG_W:
                one_axis.add("y")
    assert seen == {1, 2}
    assert {-2, -1, 0, 1, 2} <= dxs and {-2, -1, 0, 1, 2} <= dys, (dxs, dys)
    # one axis exactly at the boundary, the other above it (status 2, asserted above): `>=` on one axis alone would turn these into status 1
    assert one_axis == {"x", "y"}, one_axis


def test_orientation_family_mostly_locks(measured):
    ms = {name: m for name, _, m in measured["orientation"]}
    assert 3 * sum(m["found"] == 4 for m in ms.values()) >= 2 * len(ms)
    assert ms["rot+20"]["status"] == 0 and ms["rot+45"]["status"] == 0
    # upright, on its side, upside down: sort_top_to_bottom names a different physical anchor "top-left" each time
    tl = {name: tuple(ms[name]["anchors"][0][[0, 2]] // 300) for name in ("rot+0", "rot+90", "rot+180", "rot+270")}
    assert len(set(tl.values())) == 4, tl


def test_decoy_family_outcomes(synth, oracle, measured):
    base = measure(oracle, C.decoys_base(synth))
    assert base["found"] == 4
    real = {tuple(a) for a in base["anchors"][:3]}
    ms = {name: m for name, _, m in measured["decoys"]}
    displaced = [n for n, m in ms.items() if m["found"] >= 3 and {tuple(a) for a in m["anchors"][:3]} != real]
    nothing = [n for n, m in ms.items() if m["found"] == 3 and m["cnt"][BR_ROWS] > 0]          # the bottom-right rows were scanned and gave no anchor
    filtered = [n for n, m in ms.items() if m["cnt"][CANDIDATES] > 3 and m["found"] == 4 and (m["anchors"] == base["anchors"]).all()]
    assert displaced and nothing and filtered, (displaced, nothing, filtered)
    assert all(n.startswith("displace") or n == "filtered-and-larger" for n in displaced), displaced
    assert "window-blank" in nothing and "filtered-many" in filtered


def test_pressure_family_straddles_the_capacities(measured):
    """by the oracle's counters: every swept list has a case at half its capacity or less, one at 1.5x or more, and cases within +-2 of it on both
    sides; the case at exactly each capacity ends with four anchors; half of the cases hold a frame the search locks onto"""
    ms = [(name, m) for name, _, m in measured["pressure"]]

    def sweep(prefix, which, cap):
        v = [m["cnt"][which] for name, m in ms if name.startswith(prefix)]
        assert min(v) <= cap // 2 and max(v) >= cap + cap // 2, (prefix, v)
        near = {x - cap for x in v if abs(x - cap) <= 2}
        assert min(near) < 0 < max(near) and 0 in near, (prefix, v)
        return v
    sweep("row-", ROW_HITS, C.SCAN_ROW_PTS)
    sweep("total-", PRIMARY_HITS, C.SCAN_HMAX)
    cands = sweep("cand-", CANDIDATES, C.SCAN_MAX_CAND)
    assert min(cands) <= 8 and {14, 15, 16, 17, 18} <= set(cands)          # ... and across 16, where std::sort changes algorithm
    sweep("confirm-", CONFIRM_CHANGES, C.SCAN_CONFIRM_POS)
    locked = sum(m["found"] == 4 for _, m in ms)
    assert 2 * locked >= len(ms), locked
    for prefix, which, cap in (("row-", ROW_HITS, C.SCAN_ROW_PTS), ("total-", PRIMARY_HITS, C.SCAN_HMAX), ("cand-", CANDIDATES, C.SCAN_MAX_CAND),
                               ("confirm-", CONFIRM_CHANGES, C.SCAN_CONFIRM_POS)):
        assert any(m["cnt"][which] == cap and m["found"] == 4 and m["status"] for name, m in ms if name.startswith(prefix)), prefix
    # the row sweep's comb stands to the LEFT of two anchors on the same scan row: the anchors' hits are the last of that row's list
    for name, m in ms:
        if name.startswith("row-"):
            assert m["found"] == 4 and m["anchors"][0][0] > 2400 and m["anchors"][0][2] <= 72 <= m["anchors"][0][3], name


def test_shapes_family_has_more_rows_than_the_fast_kernels_keep(measured):
    rows = {name: m["cnt"][ROWS] for name, _, m in measured["shapes"]}
    assert sum(r > C.SCAN_MAX_ROWS for r in rows.values()) >= 3, rows
    locked = {cam.shape[:2] for _, cam, m in measured["shapes"] if m["found"] == 4 and m["status"]}
    assert locked == {cam.shape[:2] for _, cam, _ in measured["shapes"]}, locked          # every shape has a capture the search locks onto
    assert any(m["found"] < 4 for _, _, m in measured["shapes"])                          # ... and the family keeps failures too
