"""GPU: the anchor search of scan.hip.inc (k_scan_stage_rows, k_scan_confirm, k_scan_select, k_scan_final, k_scan_serial) on the hostile captures of
tests/scan_hostile_cases.py, against the oracle's co_extract -- which tests/test_scan_hostile.py pins to the reference build on the same captures.
Bit-exact: status, corners, deskewed frame. The product build and the tiny-list build (-DCIMBAR_SCAN_TINY_LISTS: nearly everything takes the serial
search) must both agree; CIMBAR_HIP_TAP_SCAN_PATH says which kernels answered."""
import os

import numpy as np
import pytest

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from oracle import pyref
from tests import scan_hostile_cases as C
from tests.scan_hostile_cases import (BR_CANDIDATES, BR_HITS, BR_ROW_HITS, BR_ROWS, CANDIDATES, CONFIRM_CHANGES, CONFIRM_LIST, HIT_CONFIRMED, PRIMARY_HITS,
                                      ROW_CHANGES, ROW_HITS, ROWS, measure)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny_list_decoder():
    """the test build of the library (libcimbar_hip_spilltest.so, -DCIMBAR_SCAN_TINY_LISTS), as in tests/test_gpu_extract.py"""
    from libcimbar_amd import build as hipbuild
    assert os.path.exists(hipbuild.OUT_SPILLTEST), "build it with `python -m libcimbar_amd.build` (or __graft_entry__.build())"
    d = D.HipDecoder(0, lib_path=hipbuild.OUT_SPILLTEST)
    yield d
    d.close()


@pytest.fixture(scope="module")
def measured(synth, oracle):
    """every mode-B family once, shared by the tests below and left unchanged"""
    return C.measure_families(synth, oracle)


def by_shape(items, limit=None):
    """indices of the captures of one shape, `limit` at most to a batch"""
    groups = {}
    for k, it in enumerate(items):
        groups.setdefault(it[1].shape, []).append(k)
    out = []
    for shape, idx in groups.items():
        step = limit or len(idx)
        out += [(shape, idx[i:i + step]) for i in range(0, len(idx), step)]
    return out


def extract_and_compare(dec, items, want_path=False, limit=None):
    """one extract_batch per capture shape; status == the oracle's, then corners and frame exactly (a failure: an all-zero frame). Returns the
    search path of every capture (CIMBAR_HIP_TAP_SCAN_PATH) when asked to."""
    paths = [None] * len(items)
    for shape, idx in by_shape(items, limit):
        batch = np.ascontiguousarray(np.stack([items[k][1] for k in idx]))
        status, corners, frames = dec.extract_batch(batch)
        if want_path:
            for j, p in enumerate(dec.tap(D.TAP_SCAN_PATH, len(idx))):
                paths[idx[j]] = int(p)
        for j, k in enumerate(idx):
            name, _, m = items[k]
            assert status[j] == m["status"], f"{name} {shape}: status {status[j]}, oracle {m['status']}"
            if m["status"]:
                assert list(corners[j]) == m["corners"], name
                assert (frames[j] == m["frame"]).all(), f"{name}: {(frames[j] != m['frame']).sum()} deskewed bytes differ"
            else:
                assert not frames[j].any(), name
    return paths


@pytest.mark.parametrize("build", ["product", "tiny-lists"])
@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_device_equals_oracle(hip_decoder, tiny_list_decoder, measured, family, build):
    if build == "product":
        extract_and_compare(hip_decoder, measured[family])
    else:          # every capture of this build takes the serial search, which has 16 slots per batch (test_slot_limit_of_the_serial_search)
        extract_and_compare(tiny_list_decoder, measured[family], limit=16)


# (selector, capacity) of every fixed list of the fast kernels the oracle counts the demand on
CAPACITIES = [(ROW_HITS, C.SCAN_ROW_PTS), (PRIMARY_HITS, C.SCAN_HMAX), (CANDIDATES, C.SCAN_MAX_CAND), (ROW_CHANGES, C.SCAN_ROW_POS),
              (CONFIRM_CHANGES, C.SCAN_CONFIRM_POS), (CONFIRM_LIST, C.SCAN_LIST), (HIT_CONFIRMED, C.SCAN_CONF_MAX), (ROWS, C.SCAN_MAX_ROWS),
              (BR_ROWS, C.SCAN_MAX_ROWS), (BR_ROW_HITS, C.SCAN_ROW_PTS), (BR_HITS, C.SCAN_HMAX), (BR_CANDIDATES, C.SCAN_MAX_CAND)]


def test_search_path_of_the_product_build(hip_decoder, measured):
    """a capture at or below half of EVERY capacity is answered by the fast kernels (path 0), one at or above 1.5x ANY capacity by k_scan_serial
    (path 1); in between only the result counts. Nothing is given up (path 2)."""
    items = measured["pressure"] + measured["shapes"] + measured["orientation"]
    paths = extract_and_compare(hip_decoder, items, want_path=True)
    low = high = 0
    for (name, _, m), p in zip(items, paths):
        assert p in (0, 1), f"{name}: path {p}"
        if all(2 * m["cnt"][sel] <= cap for sel, cap in CAPACITIES):
            assert p == 0, f"{name}: at most half of every list, yet path {p}: {m['cnt']}"
            low += 1
        elif any(2 * m["cnt"][sel] >= 3 * cap for sel, cap in CAPACITIES):
            assert p == 1, f"{name}: 1.5x a list, yet path {p}: {m['cnt']}"
            high += 1
    assert low >= 4 and high >= 4, (low, high)
    by_name = {name: p for (name, _, _), p in zip(items, paths)}
    for name in ("row-72+frame", "total-1536+frame", "cand-96+frame", "confirm-1600"):          # one per swept list
        assert by_name[name] == 1, name


@pytest.mark.parametrize("build", ["product", "tiny-lists"])
@pytest.mark.parametrize("mode", [68, 67, 66])
def test_scale_verdicts_in_every_mode(mode, build):
    """statuses 1 and 2 at is_granular_scale's boundary, in a context of each mode against the oracle built for it; modes 67 and 66 also on the
    orientation family drawn with their own frames. k_scan_final and k_scan_serial each have their own copy of the comparison: the product build
    answers these captures with the first (path 0), the tiny-list build with the second (path 1)"""
    from libcimbar_amd import build as hipbuild
    geo = geometry.for_mode(mode)
    O = pyref.oracle_lib(mode)
    synth_m = framegen.FrameSynth("cpu", mode)
    dec = D.HipDecoder(0, mode, lib_path=None if build == "product" else hipbuild.OUT_SPILLTEST)
    try:
        scale = [(name, cam, measure(O, cam, geo.FRAME_SHAPE)) for name, cam in C.scale(synth_m, mode)]
        assert {m["status"] for _, _, m in scale} == {1, 2}
        paths = extract_and_compare(dec, scale, want_path=True, limit=16)
        assert set(paths) == ({0} if build == "product" else {1}), paths
        if mode != 68:
            extract_and_compare(dec, [(name, cam, measure(O, cam, geo.FRAME_SHAPE)) for name, cam in C.orientation(synth_m)], limit=16)
    finally:
        dec.close()


def test_chain_on_rotated_captures(hip_decoder, oracle, measured):
    """scan_extract_decode_batch on the orientation family plus a capture without anchors: the chunks are co_extract + co_decode_fountain's, the
    colour-correction matrix carried capture to capture; failed captures deliver mask 0 and zero chunks"""
    items = measured["orientation"]
    cams = np.ascontiguousarray(np.stack([cam for _, cam, _ in items] + [np.zeros_like(items[0][1])]))
    hip_decoder.reset_ccm()
    total, chunks, masks, status = hip_decoder.scan_extract_decode_batch(cams)
    ccm = pyref.CoCcm()
    want_total = 0
    for k, (name, _, m) in enumerate(items):
        assert status[k] == m["status"], name
        if not m["status"]:
            assert masks[k] == 0 and not chunks[k].any(), name
            continue
        r, ch, mk, ccm = pyref.oracle_decode(m["frame"], 1 if m["status"] == 2 else 0, 2, ccm)
        assert masks[k] == mk and (chunks[k] == ch).all(), name
        want_total += r
    assert status[-1] == 0 and masks[-1] == 0 and not chunks[-1].any()
    assert total == want_total and want_total > 0


def overflowing_captures(n):
    """640x360 captures (scan rows 6 px apart) whose lower half is a comb of 1:1:3:1:1 bars, 36 hits on each of 30 rows: more than SCAN_HMAX
    together, so each takes the serial search. Above it four hand-drawn anchors, a little further apart in every capture"""
    out = []
    for k in range(n):
        img = np.zeros((360, 640, 3), np.uint8)
        for r in range(36):
            x = 8 + r * 16
            img[180:360, x:x + 2] = 255
            img[180:360, x + 4:x + 10] = 255
            img[180:360, x + 12:x + 14] = 255
        x1, y1 = 260 + 12 * k, 132 + (k % 3)
        C.bullseye(img, 40, 30, 32)
        C.bullseye(img, x1, 30, 32)
        C.bullseye(img, 40, y1, 32)
        C.bullseye(img, x1, y1, 24, kind=122)
        out.append(img)
    return out


def test_slot_limit_of_the_serial_search(hip_decoder, synth, oracle):
    """at most SCAN_SERIAL_SLOTS = 16 captures of one batch can take the serial search; the rest are reported as failures
    (the documented status -1, a zero frame, path 2) -- and the slot counter is re-armed for the next call"""
    cams = overflowing_captures(20)
    want = [measure(oracle, cam) for cam in cams]
    assert all(m["cnt"][PRIMARY_HITS] > C.SCAN_HMAX for m in want), [m["cnt"][PRIMARY_HITS] for m in want]
    assert sum(m["status"] != 0 for m in want) >= 10          # most of them have a quad to get right
    status, corners, frames = hip_decoder.extract_batch(np.ascontiguousarray(np.stack(cams)))
    path = hip_decoder.tap(D.TAP_SCAN_PATH, 20)
    answered = 0
    for k, m in enumerate(want):
        if path[k] == 1:
            assert status[k] == m["status"], k
            if m["status"]:
                assert list(corners[k]) == m["corners"] and (frames[k] == m["frame"]).all(), k
            answered += 1
        else:
            # (given up: the failure the header documents as status -1, never a success; nothing of the capture is delivered)
            assert path[k] == 2 and status[k] == -1 and not frames[k].any(), (k, path[k], status[k])
    assert answered == 16, answered
    status, corners, frames = hip_decoder.extract_batch(np.ascontiguousarray(np.stack(cams[:3])))
    assert list(hip_decoder.tap(D.TAP_SCAN_PATH, 3)) == [1, 1, 1]
    assert [int(s) for s in status] == [m["status"] for m in want[:3]]
