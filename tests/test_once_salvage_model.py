"""CPU: tear salvage's rule (tests/once_salvage_model.py, written from include/cimbar_hip.h "Tear salvage") on hand-made records, on both
sides of every clause's edge; the margins, records and plans of tests/once_salvage_cases.py that tests/test_gpu_once_salvage.py relies on;
the oracle's per-frame decode of the wiped captures (incomplete) and of their clean frames (complete); and that the header, the library
and the binding name the same things."""
import numpy as np
import pytest

from libcimbar_amd import geometry, modeb
from oracle import pyref
from tests import once_salvage_cases as SC
from tests import once_salvage_model as SM
from tests import once_tear_model as TM
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM

MODE = 66      # the hand-made records: 69 grid rows, 80 grid columns
L0, L1 = 69, 80
FULL = geometry.for_mode(MODE).FULL_MASK


def test_the_header_the_library_and_the_binding_name_the_same_things():
    import os
    import re
    from libcimbar_amd import decoder as D
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cimbar_hip.h")).read()
    assert re.search(r"\bCIMBAR_HIP_TAP_ONCE_SALVAGE\s*=\s*35\b", header) and D.TAP_ONCE_SALVAGE == 35
    lib = D.load_library()
    for name in ("cimbar_hip_set_once_tear_salvage", "cimbar_hip_get_once_tear_salvage"):
        assert name in D.EXPORTS and re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(lib, name) is not None
    for name in ("set_once_tear_salvage", "get_once_tear_salvage", "tap_once_salvage"):
        assert callable(getattr(D.HipDecoder, name))
    assert (SM.GUARD_DEFAULT, SM.GUARD_MAX, SM.GMAX) == (1, 16, 8)      # what the header states
    assert "guard_lines -1 resolves to 1; 0 .. 16 are legal" in header and "fewer than 8 members" in header
    assert TM.lines(MODE, 0)[1] == L0 and TM.lines(MODE, 1)[1] == L1


def test_guard_resolution():
    assert SM.resolve(-1) == 1 and SM.resolve(0) == 0 and SM.resolve(1) == 1 and SM.resolve(16) == 16
    for bad in (-2, 17, 100):
        with pytest.raises(ValueError):
            SM.resolve(bad)
    assert SM.effective(1, 1, 0, True, False) and SM.effective(1, 1, 2, False, True)
    assert not SM.effective(0, 1, 0, True, True) and not SM.effective(1, 0, 0, True, True)
    assert not SM.effective(1, 1, -1, True, True) and not SM.effective(1, 1, 0, False, False)


def test_sides_by_orientation_axis_and_guard():
    # o = 0: P on the low lines
    assert SM.sides(MODE, (0, 20, 20, 49), 1) == ((0, 0, 19), (0, 21, L0))
    assert SM.sides(MODE, (0, 20, 20, 49), 0) == ((0, 0, 20), (0, 20, L0))
    assert SM.sides(MODE, (0, 20, 20, 49), 16) == ((0, 0, 4), (0, 36, L0))
    # o = 1: P on the high lines
    assert SM.sides(MODE, (1, 20, 20, 49), 1) == ((0, 21, L0), (0, 0, 19))
    # axis 1: the grid columns
    assert SM.sides(MODE, (2, 30, 30, 50), 3) == ((1, 0, 27), (1, 33, L1))
    assert SM.sides(MODE, (3, 30, 30, 50), 3) == ((1, 33, L1), (1, 0, 27))
    # an empty side, and the last guard that leaves a line
    assert SM.sides(MODE, (0, 2, 2, 67), 2) == (None, (0, 4, L0))
    assert SM.sides(MODE, (0, 2, 2, 67), 1) == ((0, 0, 1), (0, 3, L0))
    assert SM.sides(MODE, (0, 60, 60, 9), 9) == ((0, 0, 51), None)
    assert SM.sides(MODE, (0, 60, 60, 9), 8) == ((0, 0, 52), (0, 68, L0))
    assert SM.sides(MODE, (1, 16, 16, 53), 16) == ((0, 32, L0), None)


def _rec(n, cands):
    rec = np.tile(np.array(TM.NO_TEAR, np.int32), (n, 1))
    for k, r in cands.items():
        rec[k] = r
    return rec


def test_partials_by_orientation_and_role():
    # [0] T [2 3] T [5]: capture 1 torn with o = 0, capture 4 with o = 1
    members = [[0], [1], [2, 3], [4], [5]]
    rec = _rec(6, {1: (0, 20, 20, 49), 4: (1, 30, 39, 30)})
    roles = np.array([RM.REP, RM.FALLBACK, RM.REP, RM.FALLBACK, RM.FALLBACK, RM.REP])
    parts = SM.partials(MODE, members, rec, roles, 1)
    assert parts[0] == (None, (1, 0, 0, 19))                             # following: capture 1's P side, low
    assert parts[1] == (None, None) and parts[3] == (None, None)         # a candidate's own run
    assert parts[2] == ((1, 0, 21, L0), (4, 0, 31, L0))                  # preceding: capture 1's N side; following: capture 4's P side, high (o = 1)
    assert parts[4] == ((4, 0, 0, 29), None)                             # preceding: capture 4's N side, low (o = 1)
    # a torn candidate (role 3) and a skipped member give nothing; a fallback that is no candidate neither
    roles[1] = TM.TORN
    parts = SM.partials(MODE, members, rec, roles, 1)
    assert parts[0] == (None, None) and parts[2] == (None, (4, 0, 31, L0))
    roles[1] = RM.FALLBACK
    rec[1] = TM.NO_TEAR
    assert SM.partials(MODE, [[0], [1], [2, 3], [4], [5]], rec, roles, 1)[0] == (None, None)
    # an empty side gives no partial, the other side of the same candidate still does
    rec = _rec(3, {1: (0, 2, 2, 67)})
    roles = np.array([RM.REP, RM.FALLBACK, RM.REP])
    assert SM.partials(MODE, [[0], [1], [2]], rec, roles, 2) == [(None, None), (None, None), ((1, 0, 4, L0), None)]
    assert SM.partials(MODE, [[0], [1], [2]], rec, roles, 1) == [(None, (1, 0, 0, 1)), (None, None), ((1, 0, 3, L0), None)]


def test_qualifies_and_tried():
    members = [[0], [1], [2, 3], [4], [5], [6]]
    rec = _rec(7, {1: (0, 20, 20, 49), 4: (0, 30, 30, 39)})
    roles = np.array([RM.REP, RM.FALLBACK, RM.REP, RM.FALLBACK, RM.FALLBACK, RM.REP, RM.REP])
    parts = SM.partials(MODE, members, rec, roles, 1)
    masks = np.array([FULL & ~1, 0, FULL & ~2, FULL & ~6, 0, FULL, FULL & ~1])
    # run 0: one member and a partial; run 2: two members; run 4: complete; run 5: one member, incomplete, no partial; the candidates: never
    assert SM.qualifies(MODE, members, rec, masks, parts) == [True, False, True, False, False, False]
    assert SM.tried(MODE, members, rec, masks, parts) == [True, False, True, False, False, False]
    masks[3] = FULL                                                      # pass 2 completes run 2: it qualifies and is not tried
    assert SM.qualifies(MODE, members, rec, masks, parts) == [True, False, True, False, False, False]
    assert SM.tried(MODE, members, rec, masks, parts) == [True, False, False, False, False, False]
    masks[0] = FULL                                                      # a complete representative: nothing to do
    assert SM.tried(MODE, members, rec, masks, parts) == [False] * 6
    masks[5] = FULL & ~8                                                 # run 4 = [5] now incomplete, with capture 4 in front of it
    assert SM.tried(MODE, members, rec, masks, parts) == [False, False, False, False, True, False]
    rows = SM.tap_rows(7, members, SM.tried(MODE, members, rec, masks, parts), parts)
    assert rows[4].tolist() == [4, 0, 31, L0, -1, -1, 0, 0]
    assert all(rows[r].tolist() == [-1, -1, 0, 0, -1, -1, 0, 0] for r in (0, 1, 2, 3, 5, 6))


def test_group_order_and_the_cap():
    prec, foll = (9, 0, 31, L0), (20, 0, 0, 19)
    assert SM.group([10, 11], (prec, foll)) == [(10, None), (11, None), (9, (0, 31, L0)), (20, (0, 0, 19))]
    assert SM.group([10], (None, foll)) == [(10, None), (20, (0, 0, 19))]
    six, seven, eight = list(range(10, 16)), list(range(10, 17)), list(range(10, 18))
    assert len(SM.group(six, (prec, foll))) == 8 and SM.group(six, (prec, foll))[6:] == [(9, (0, 31, L0)), (20, (0, 0, 19))]
    assert SM.group(seven, (prec, foll))[7:] == [(9, (0, 31, L0))]         # room for one: the preceding partial
    assert SM.group(seven, (None, foll))[7:] == [(20, (0, 0, 19))]
    assert SM.group(eight, (prec, foll)) == [(k, None) for k in eight]     # GMAX is full: no partial
    # the tap names only the partials that joined
    rows = SM.tap_rows(3, [seven, eight], [True, True], [(prec, foll), (prec, foll)])
    assert rows[0].tolist() == [9, 0, 31, L0, -1, -1, 0, 0] and rows[1].tolist() == [-1, -1, 0, 0] * 2 and rows[2].tolist() == [-1, -1, 0, 0] * 2


def test_combined_cells_with_participation():
    geo = geometry.for_mode(MODE)
    n = geo.NCELLS
    line = TM.lines(MODE, 0)[0]
    plane = lambda v: np.full(geo.IMG_H * geo.IMG_W // 8, v, np.uint8)
    light = int(np.argmin([bin(int(t)).count("1") for t in modeb.TILE_HASHES]))       # a tile nearer to an all-zero window than to an all-one window
    assert bin(int(modeb.TILE_HASHES[light])).count("1") < 32
    # member 0 (capture 5) full, all-one bit plane; the partials (captures 4 and 6), all-zero planes: lines [40, 69) and [0, 30)
    grp = [(5, None), (4, (0, 40, L0)), (6, (0, 0, 30))]
    who = SM.participation(MODE, grp)
    assert who[0].all() and (who[1] == (line >= 40)).all() and (who[2] == (line < 30)).all()
    assert not (who[1] & who[2]).any() and (who.sum(axis=0)[(line >= 30) & (line < 40)] == 1).all()
    bit = {5: plane(0xFF), 4: plane(0), 6: plane(0)}
    drift = {k: np.zeros((n, 2), np.int8) for k in bit}
    flood = {k: 0 for k in bit}
    sym = {5: np.full(n, light, np.uint8), 4: np.full(n, light, np.uint8), 6: np.full(n, (light + 1) % 16, np.uint8)}
    col = {5: np.full(n, 1, np.uint8), 4: np.full(n, 2, np.uint8), 6: np.full(n, 1, np.uint8)}
    cells, margins, disputed = SM.combine_cells(MODE, bit, sym, col, drift, flood, grp)
    mid, hi, lo = (line >= 30) & (line < 40), line >= 40, line < 30
    # one participant: its symbol and colour, undisputed
    assert (cells[mid] == ((1 << 4) | light)).all() and (margins[mid] == SM.CM.MARGIN_NONE).all()
    # members 0 and 1: equal symbols, colours 1 and 2 tie; member 1's window is nearer to the symbol's tile, so its colour wins
    assert (cells[hi] == ((2 << 4) | light)).all() and (margins[hi] == SM.CM.MARGIN_NONE).all()
    # members 0 and 2: the symbols differ, so the vote decides and the margin is set; the colours agree
    assert (margins[lo] != SM.CM.MARGIN_NONE).all() and ((cells[lo] >> 4) == 1).all() and disputed
    # the tie index is the position in the group's order: three colours, the partials equally near -- the preceding partial (position 1)
    # wins over the following one (position 2) whatever their capture indices are
    grp3 = [(5, None), (6, (0, 0, L0)), (4, (0, 0, L0))]
    col3 = {5: np.full(n, 1, np.uint8), 6: np.full(n, 3, np.uint8), 4: np.full(n, 2, np.uint8)}
    sym3 = {k: np.full(n, light, np.uint8) for k in bit}
    cells3, _, _ = SM.combine_cells(MODE, bit, sym3, col3, drift, flood, grp3)
    assert (cells3 == ((3 << 4) | light)).all()
    # no participant differs anywhere: not disputed
    same = {k: np.full(n, 1, np.uint8) for k in bit}
    assert SM.combine_cells(MODE, bit, sym3, same, drift, flood, grp)[2] is False


# ------------------------------------------------------------------------------------------------ the cases' premises
def _plan(mode, frames, min_agree, line, max_run=0):
    sigs, agree, runs, members, _ = RM.plan(mode, frames, min_agree_permille=min_agree, max_run=max_run)
    rec = TM.records(mode, sigs, runs, members, 0, line)
    return sigs, agree, runs, members, rec


def _after_pass_1(mode, runs, members, rec, incomplete):
    """lists, roles and masks as they come out when exactly the captures in `incomplete` (and every torn candidate's decode) are not full"""
    full = geometry.for_mode(mode).FULL_MASK
    l1 = TM.list1(members, rec)
    masks1 = {k: (full & ~1 if k in incomplete else full) for k in l1}
    l2, torn = TM.second(mode, runs, members, rec, masks1)
    masks = np.array([masks1.get(k, 0 if k in TM.candidates(rec) else (full & ~1 if k in incomplete else full)) for k in range(len(runs))])
    return l1, l2, torn, TM.roles(len(runs), runs, l1, l2, torn), masks


@pytest.mark.parametrize("mode", SC.MODES)
def test_s1_margins_records_and_plan(mode):
    geo = geometry.for_mode(mode)
    sigs, agree, runs, members, rec = _plan(mode, SC.s1(mode), SC.MIN_AGREE, SC.LINE)
    pm = [int(a) * 1000 // geo.NCELLS for a in agree]
    assert pm == SC.S1_AGREE[mode] and runs.tolist() == SC.S1_RUNS
    assert min(p for p in pm if p >= SC.MIN_AGREE) == 1000 and max(p for p in pm if p < SC.MIN_AGREE) <= SC.MIN_AGREE - 63
    assert TM.candidates(rec) == [1, 4] and (tuple(rec[1]), tuple(rec[4])) == SC.S1_RECORDS[mode]
    # the same records at tear skipping's default line_permille, but with a thin margin: the wipe's lines
    assert TM.records(mode, sigs, runs, members, 0, 750).tolist() == rec.tolist()
    for k in (1, 4):
        s = int(rec[k][1])
        vp, vn = TM.line_permilles(mode, 0, sigs[k], sigs[k - 1]), TM.line_permilles(mode, 0, sigs[k], sigs[k + 1])
        # (the lines through the wipe: 758 or more against wipe8(A) in front of capture 1, 750 or more against wipe8(C) behind capture 4)
        assert min(vp[:s].min(), vn[s + 1:].min()) >= SC.LINE + (108 if k == 1 else 100)
        assert max(vn[:s].max(), vp[s + 1:].max()) <= SC.LINE - 108
    l1, l2, torn, roles, masks = _after_pass_1(mode, runs, members, rec, {0, 5})
    assert (l1, l2, torn) == (SC.S1_LIST1, SC.S1_LIST2, [])
    L = geo.DIM_Y
    parts = SM.partials(mode, members, rec, roles, 1)
    assert parts[0] == (None, (1, 0, 0, int(rec[1][1]) - 1)) and parts[4] == ((4, 0, int(rec[4][1]) + 1, L), None)
    assert SM.tried(mode, members, rec, masks, parts) == SC.S1_TRIED
    # the wipe (the middle 28 % of the lines) lies inside both ranges
    line = TM.lines(mode, 0)[0]
    wiped = np.unique(line[RM.signature(mode, SC.s1(mode)[0]) != RM.signature(mode, RC.clean(mode)[1][0])])
    assert wiped.min() >= int(rec[4][1]) + 1 and wiped.max() < int(rec[1][1]) - 1


@pytest.mark.parametrize("mode", SC.MODES)
def test_further_cases_plans(mode):
    geo = geometry.for_mode(mode)
    L = geo.DIM_Y
    # one candidate between two incomplete runs of one
    _, agree, runs, members, rec = _plan(mode, SC.both_sides(mode), SC.MIN_AGREE, SC.LINE)
    assert runs.tolist() == SC.BOTH_RUNS and TM.candidates(rec) == [1] and rec[1][0] == 0
    l1, l2, torn, roles, masks = _after_pass_1(mode, runs, members, rec, {0, 2})
    assert (l1, l2, torn) == ([0, 2], [1], [])
    s = int(rec[1][1])
    parts = SM.partials(mode, members, rec, roles, 1)
    assert parts == [(None, (1, 0, 0, s - 1)), (None, None), ((1, 0, s + 1, L), None)]
    assert SM.tried(mode, members, rec, masks, parts) == SC.BOTH_TRIED
    # the tried pair with a torn capture behind it
    _, agree, runs, members, rec = _plan(mode, SC.pair_and_partial(mode), SC.PAIR_MIN_AGREE, SC.PAIR_LINE)
    pm = [int(a) * 1000 // geo.NCELLS for a in agree]
    assert runs.tolist() == SC.PAIR_RUNS and TM.candidates(rec) == [2] and rec[2][0] == 0
    assert min(pm[0], pm[3]) >= SC.PAIR_MIN_AGREE + 20 and max(pm[1], pm[2]) <= SC.PAIR_MIN_AGREE - 100
    l1, l2, torn, roles, masks = _after_pass_1(mode, runs, members, rec, {0, 1})
    assert (l1, l2, torn) == ([0, 3], [1, 2], [])
    parts = SM.partials(mode, members, rec, roles, 1)
    assert parts[0] == (None, (2, 0, 0, int(rec[2][1]) - 1)) and parts[2] == ((2, 0, int(rec[2][1]) + 1, L), None)   # (run 2 is complete: its partial is never used)
    assert SM.tried(mode, members, rec, masks, parts) == SC.PAIR_TRIED
    assert SM.group(members[0], parts[0]) == [(0, None), (1, None), (2, (0, 0, int(rec[2][1]) - 1))]
    # the full run of eight
    _, agree, runs, members, rec = _plan(mode, SC.full_run(mode), SC.MIN_AGREE, SC.LINE, max_run=8)
    assert runs.tolist() == SC.FULL_RUNS and TM.candidates(rec) == [8]
    l1, l2, torn, roles, masks = _after_pass_1(mode, runs, members, rec, set(range(8)))
    assert l1 == [3, 9] and l2 == [0, 1, 2, 4, 5, 6, 7, 8]
    parts = SM.partials(mode, members, rec, roles, 1)
    tried = SM.tried(mode, members, rec, masks, parts)
    assert parts[0][1] is not None and tried == SC.FULL_TRIED
    assert SM.group(members[0], parts[0]) == [(k, None) for k in range(8)]
    assert (SM.tap_rows(10, members, tried, parts) == np.array(SM.NO_PARTIAL * 2)).all()


@pytest.mark.parametrize("mode", SC.MODES)
def test_the_oracle_decodes_the_wiped_captures_incompletely_and_their_frames_completely(mode):
    full = geometry.for_mode(mode).FULL_MASK
    payload, f = RC.clean(mode)
    decode = lambda frame: pyref.oracle_decode(np.ascontiguousarray(frame), 0, 2, None, mode=mode)
    for k in range(3):
        r, chunks, mask, _ = decode(f[k])
        assert mask == full and (np.asarray(chunks).reshape(-1) == np.asarray(payload[k]).reshape(-1)).all(), k
    s1, both, run8 = SC.s1(mode), SC.both_sides(mode), SC.full_run(mode)
    for name, frame in (("s1[0]", s1[0]), ("s1[5]", s1[5]), ("both[0]", both[0]), ("both[2]", both[2]), ("full[0]", run8[0]), ("full[3]", run8[3]),
                        ("full[7]", run8[7])):
        assert decode(frame)[2] != full, name
