"""The fast-path theorem of the parallel symbol pass (DESIGN.md "K2 `k_symbols`") on the line between its two outcomes, on the CPU: the numpy
restatement of the condition (tests/fast_path_model.py) and the oracle's priority-queue flood (co_symbol_pass) on the frames of
tests/fast_path_cases.py, in every mode.

  * the model's flag is 0 exactly on the cases that are meant to stay on the fast path;
  * on those, the oracle's flood visits every cell at its undrifted position with the model's parallel symbol -- frames with thousands of
    inexact cells, side windows that tie the centre, corner windows that beat it, and centre hashes equidistant from two tiles;
  * on the flagged cases of sets 3 and 4 (one violating cell each) the flood drifts or differs somewhere in the set (the count is printed: in
    every mode it was every frame of both sets when this was written);
  * the floors of sets 1 and 2: what makes these frames a test of `<`, of the seeds' eight windows and of the first-minimum tile.

Mutation checks. Each was done twice when this was written: once on the frames as they are (the mutant judges frames the true rule built:
test_mutant_* below, kept as tests), and once with the mutant in place for a whole run of this file, so that it built the frames too (by hand,
9 of 61 tests failed each time):
  * the model's `<` made `<=` (fast_path_model.STRICT = False). On the frames as they are: all four boundary frames and the seed-neighbours
    frame come out flagged, in every mode. For a whole run: set 1 fails in every mode (test_boundary_floors: the builder can no longer leave a
    tie, "side_ties 0 < 500") and set 4 in modes 67, 66, 4 and 8 (test_flag: the seed-neighbours frame is flagged by a cell with side == dc;
    in mode 68 the draw held no tie);
  * the seed rule made "sides only" (fast_path_model.SEEDS_LOOK_AT_CORNERS = False). On the frames as they are: none of the eight seed frames
    is flagged, in every mode, while the oracle's flood drifts at the seed on each. For a whole run: test_flag[4] fails in every mode at its
    first seed frame ("flag 0, violating cells: []"), and test_theorem_against_the_flood[1] in modes 68, 67, 4 and 8: the repair leaves seeds
    whose corner window beats the centre, and the flood drifts there on a frame the mutant calls unflagged."""
import numpy as np
import pytest

from tests import fast_path_cases as K
from tests import fast_path_model as M

MODES = K.MODES
first_difference = K.first_difference


@pytest.mark.parametrize("set_no", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_flag(mode, set_no):
    T = M.tables(mode)
    for case in K.cases(mode, set_no):
        res = case.result
        bad = np.flatnonzero(res.violates)
        assert bool(res.flag) == case.flagged, f"{case}: flag {res.flag}, violating cells: {[res.describe(T, i) for i in bad[:4]]}"
        if case.flagged:
            assert bad.tolist() == sorted(case.cells), f"{case}: {[res.describe(T, i) for i in bad[:4]]}"


@pytest.mark.parametrize("set_no", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_theorem_against_the_flood(mode, set_no):
    T = M.tables(mode)
    moved = 0
    flagged = [c for c in K.cases(mode, set_no) if c.flagged]
    for case in K.cases(mode, set_no):
        sym, pos = K.oracle_flood(case)
        if case.flagged:
            moved += bool((pos != T.xy).any() or (sym != case.result.symbols).any())
        else:
            bad = first_difference(case, sym, case.result.symbols, pos, T.xy)
            assert bad is None, "the flood leaves the parallel result on an unflagged frame -- " + bad
    if flagged:
        print(f"mode {mode} set {set_no}: the flood drifts or differs on {moved} of {len(flagged)} flagged frames")
        assert moved >= 1, f"mode {mode} set {set_no}: no flagged frame moves the flood: the set does not show that its flags are needed"


@pytest.mark.parametrize("mode", MODES)
def test_boundary_floors(mode):
    cases = K.boundary(mode)
    assert [c.name for c in cases] == [f"boundary-{f}" for f in K.BOUNDARY_FLIPS]
    for case in cases:
        counts = M.class_counts(case.result, mode)
        print(case, counts)
        assert counts["violating"] == 0, case
    counts = M.class_counts(cases[K.BOUNDARY_FLIPS.index(20)].result, mode)
    for what, floor in K.FLOORS.items():
        assert counts[what] >= floor, f"mode {mode} boundary-20: {what} {counts[what]} < {floor}: change the seed, not the floor"


@pytest.mark.parametrize("mode", MODES)
def test_queue_floors(mode):
    geo = M.tables(mode).geo
    for case, flips in zip(K.queue_stress(mode), K.QUEUE_FLIPS):
        res = case.result
        counts = M.class_counts(res, mode)
        print(case, counts)
        assert counts["inexact"] == geo.NCELLS and counts["violating"] == 0, (case, counts)
        strip, slot = M.queue_slots(res, mode)
        per_strip = np.bincount(strip, minlength=strip.max() + 1)
        assert (np.bincount(strip, weights=slot >= 0) == per_strip).all()
        # every cell of a wavefront's rows queued: 8 x 112 = 896 in the full strips of the 112-column modes, the queue's capacity, walked in 14 turns
        assert slot.max() + 1 == M.QUEUE_ROWS * geo.DIM_X
        last = strip.max()
        rows_last = geo.DIM_Y - last * M.QUEUE_ROWS
        assert rows_last == {68: 8, 67: 6, 66: 5, 4: 8, 8: 8}[mode]
        assert per_strip[last] == (slot[strip == last].max() + 1)


@pytest.mark.parametrize("mode", MODES)
def test_locations(mode):
    """set 3's cells are where they are meant to be, on the planes the device will see"""
    T = M.tables(mode)
    geo = T.geo
    loc = K.locations(mode)
    by_name = {c.name: c for c in K.one_cell(mode)}
    assert set(by_name) == set(loc) and ("row-68" in loc) == (mode == 66)
    assert loc["cell-0"] == 0 and loc["last-cell"] == geo.NCELLS - 1
    assert T.col[loc["last-column"]] == geo.DIM_X - 1
    assert T.row[loc["last-strip"]] // M.QUEUE_ROWS == (geo.DIM_Y - 1) // M.QUEUE_ROWS
    assert (T.xy[loc["word-straddle"], 0] & 31) > 24
    if mode == 66:
        assert T.row[loc["row-68"]] == 68
    for name, case in by_name.items():
        res = case.result
        c = loc[name]
        assert res.dc[c] != 0 and res.other[c] == res.dc[c] - 1, f"{case}: {res.describe(T, c)}"
    strip, slot = M.queue_slots(by_name["queue-second-turn"].result, mode)
    assert 64 <= slot[loc["queue-second-turn"]] < 128, slot[loc["queue-second-turn"]]


@pytest.mark.parametrize("mode", MODES)
def test_seed_frames(mode):
    T = M.tables(mode)
    cases = K.seed_cases(mode)
    assert len(cases) == 9
    for k, case in enumerate(cases[:8]):
        res, s = case.result, int(T.seeds[k])
        assert case.cells == (s,) and T.is_seed[s]
        assert res.dc[s] != 0 and res.corner[s] < res.dc[s] <= res.side[s], f"{case}: {res.describe(T, s)}"
    res = cases[8].result
    assert len(set(cases[8].cells)) == 8 and not T.is_seed[list(cases[8].cells)].any()
    for c in cases[8].cells:
        assert res.dc[c] != 0 and res.corner[c] < res.dc[c] <= res.side[c], f"{cases[8]}: {res.describe(T, c)}"
    assert not res.violates[T.seeds].any()


def test_hashes_and_keys_on_a_clean_plane():
    """the model's own parts against the oracle's tables: a clean plane's centre hashes are tile hashes, at distance 0, and the model's windows
    are the ones the flood reads (its symbols on a clean plane are the centre tiles)"""
    for mode in (68, 66):
        T = M.tables(mode)
        plane = K.clean_plan(mode)
        win = M.cell_windows(plane, mode)
        h = M.window_hashes(win)
        keys = M.window_keys(win, mode)
        exact = (keys[:, 4] >> 4) == 0
        assert exact.mean() > 0.98
        assert (h[exact, 4] == T.hashes[keys[exact, 4] & 15]).all()
        # distances from the hashes themselves: popcount(h ^ tile)
        x = h[:, :, None] ^ T.hashes[None, None, :]
        pop = np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).reshape(x.shape + (64,)).sum(-1)
        assert (pop == M.window_distances(win, mode)).all()


@pytest.fixture
def mutant(monkeypatch):
    def apply(**kw):
        for k, v in kw.items():
            monkeypatch.setattr(M, k, v)
    return apply


@pytest.mark.parametrize("mode", MODES)
def test_mutant_le_is_caught(mode, mutant):
    """`<=` for `<`: every boundary frame and the seed-neighbours frame would be flagged"""
    cases = K.boundary(mode) + K.seed_cases(mode)[8:]
    mutant(STRICT=False)
    for case in cases:
        assert M.evaluate(case.plane, mode).flag == 1, case


@pytest.mark.parametrize("mode", MODES)
def test_mutant_sides_only_seeds_is_caught(mode, mutant):
    """seeds that look at their side windows only: none of the eight seed frames would be flagged -- and the flood does move on them"""
    T = M.tables(mode)
    cases = K.seed_cases(mode)[:8]
    mutant(SEEDS_LOOK_AT_CORNERS=False)
    for case in cases:
        assert M.evaluate(case.plane, mode).flag == 0, case
        sym, pos = K.oracle_flood(case)
        assert (pos[list(case.cells)] != T.xy[list(case.cells)]).any(), f"{case}: the flood does not drift at the seed"
