"""GPU: the parallel symbol pass (k_symbols) on the line between "this frame is the reference's result as it stands" and "flag it for the flood
kernels" -- the frames of tests/fast_path_cases.py, held against the numpy restatement of the condition (tests/fast_path_model.py) and against
the oracle, in every mode. One test per set:

  1 boundary   unflagged frames with thousands of inexact cells, side windows that tie the centre (`<`, not `<=`), corner windows that beat it
               (ordinary cells do not look at them) and centre hashes equidistant from two tiles (the first minimum wins)
  2 queue      every cell inexact, none violating: each wavefront's queue at its capacity, the last strip partial
  3 one cell   frames flagged by one cell alone, whose best other window is one closer than its centre: cell 0, the last cell, the last column,
               the last strip, row 68 of mode 66, a block that straddles a plane word, a cell in the second turn of the queue walk
  4 seeds      a corner window beats the centre at one seed (flagged) / at the seeds' non-seed neighbours (unflagged)
  5 split      all of them, repeated to 160 frames: the chain as two half-batches on two streams

Per frame: TAP_BITPLANE is the oracle's plane (the precondition: the device looks at the plane the model was given); TAP_FLOOD is zero exactly
where the model's flag is, and TAP_FLOOD_PATH is 0 exactly there; TAP_SYMBOLS is the model's parallel result on unflagged frames; TAP_SYMBOLS and
TAP_DRIFT are the oracle's on every frame (an unflagged frame's drift reads as zero); masks and chunks are oracle_decode's, the colour matrix
carried in order."""
import numpy as np
import pytest

from libcimbar_amd import decoder as D
from tests import fast_path_cases as K
from tests import fast_path_model as M
from tests.fast_path_cases import first_difference

pytestmark = pytest.mark.gpu

MODES = K.MODES


def run(mode, frames):
    dec = D.HipDecoder(0, mode)
    try:
        n = len(frames)
        dec.reset_ccm()
        total, chunks, masks = dec.decode_batch(frames, should_preprocess=0)
        taps = {t: dec.tap(t, n) for t in (D.TAP_BITPLANE, D.TAP_FLOOD, D.TAP_FLOOD_PATH, D.TAP_SYMBOLS, D.TAP_DRIFT)}
        return np.array(chunks, copy=True), np.array(masks, copy=True), taps
    finally:
        dec.close()


def check_frame(case, where, taps, k):
    """frame k of a batch holds `case`: plane, flag, path, symbols and drift"""
    T = M.tables(case.mode)
    res = case.result
    plane = taps[D.TAP_BITPLANE][k]
    bad = np.flatnonzero(plane != case.packed)
    if bad.size:
        y, x = divmod(int(bad[0]) * 8, T.geo.IMG_W)
        raise AssertionError(f"{case}{where}: {bad.size} bit plane bytes differ from the oracle's, first at row {y}, pixels {x}..{x + 7}")
    flood, path = int(taps[D.TAP_FLOOD][k]), int(taps[D.TAP_FLOOD_PATH][k])
    viol = np.flatnonzero(res.violates)
    if res.flag:
        assert flood != 0 and path != 0, f"{case}{where}: the flag is lost (flood {flood}, path {path}); violating {res.describe(T, int(viol[0]))}"
    else:
        closest = int(np.argmin(np.where(res.dc != 0, res.other.astype(np.int64) - res.dc, 1 << 20)))
        assert flood == 0 and path == 0, (f"{case}{where}: flagged (flood {flood}, path {path}) though no cell violates; "
                                          f"the closest is {res.describe(T, closest)}")
    sym, drift = taps[D.TAP_SYMBOLS][k], taps[D.TAP_DRIFT][k].astype(np.int32)
    if not res.flag:
        bad = first_difference(case, sym, res.symbols)
        assert bad is None, f"{where}: not the model's parallel symbols -- {bad}"
    wsym, wpos = K.oracle_flood(case)
    bad = first_difference(case, sym, wsym, T.xy + drift, wpos)
    assert bad is None, f"{where}: not the oracle's flood -- {bad}"


def check_set(mode, set_no):
    cases = K.cases(mode, set_no)
    assert len(cases) <= 30
    frames = np.ascontiguousarray(np.stack([c.frame for c in cases]))
    chunks, masks, taps = run(mode, frames)
    want = K.oracle_decode(mode, set_no)
    for k, (case, w) in enumerate(zip(cases, want)):
        check_frame(case, "", taps, k)
        # the whole decode's stage outputs are the plane's flood (the oracle against itself: the two entry points agree)
        wsym, wpos = K.oracle_flood(case)
        assert (w["sym"] == wsym).all() and (w["pos"] == wpos).all(), case
        assert int(masks[k]) == w["mask"], f"{case}: mask {int(masks[k]):#x} for {w['mask']:#x}"
        got = np.asarray(chunks[k]).reshape(-1)
        bad = np.flatnonzero(got != w["chunks"].reshape(-1))
        assert bad.size == 0, f"{case}: {bad.size} chunk bytes differ, first at {int(bad[0])}"
    return taps


@pytest.mark.parametrize("mode", MODES)
def test_boundary_frames_stay_on_the_fast_path(mode):
    taps = check_set(mode, 1)
    assert not taps[D.TAP_FLOOD].any()


@pytest.mark.parametrize("mode", MODES)
def test_full_queues_stay_on_the_fast_path(mode):
    taps = check_set(mode, 2)
    assert not taps[D.TAP_FLOOD].any()


@pytest.mark.parametrize("mode", MODES)
def test_one_violating_cell_flags_its_frame(mode):
    taps = check_set(mode, 3)
    assert taps[D.TAP_FLOOD].all() and taps[D.TAP_FLOOD_PATH].all()


@pytest.mark.parametrize("mode", MODES)
def test_seeds_look_at_eight_windows_and_other_cells_at_four(mode):
    taps = check_set(mode, 4)
    assert taps[D.TAP_FLOOD][:8].all() and taps[D.TAP_FLOOD][8] == 0


@pytest.mark.parametrize("mode", [68, 66])
def test_split_batch(mode):
    unique, index = K.split_batch(mode)
    assert len(index) == K.SPLIT_FRAMES and len(unique) <= 30
    frames = np.stack([c.frame for c in unique])[index]
    chunks, masks, taps = run(mode, frames)
    for k, u in enumerate(index):
        check_frame(unique[u], f" (frame {k} of {len(index)})", taps, k)
