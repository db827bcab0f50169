"""CPU: tear skipping's rule (tests/once_tear_model.py) clause by clause on hand-made signatures, on both sides of every edge; the per-line
margins of the inputs the GPU tests use (tests/once_tear_cases.py); and the roles and lists those inputs must produce.

The margins: on a torn capture every line on a neighbour's side agrees with that neighbour on at least 900 permille of its cells and with the
other neighbour on at most 600; the line the tear crosses in mid-cell lies between the two groups -- above every other-side line of its
capture and below every same-side line. (Seen: 1000, at most 430, and 526 .. 705 for the crossed line.)"""
import numpy as np
import pytest

from libcimbar_amd import geometry
from tests import once_tear_cases as TC
from tests import once_tear_model as TM
from tests import repeat_skip_model as RM
from tests import stitch_cases as SC

MODE = 66      # the hand-made signatures: 69 grid rows, 80 grid columns


def test_the_header_the_binding_and_the_model_name_the_same_things():
    import os
    import re
    from libcimbar_amd import decoder as D
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cimbar_hip.h")).read()
    assert re.search(r"\bCIMBAR_HIP_ONCE_TORN\s*=\s*3\b", header) and D.ONCE_TORN == TM.TORN == 3
    assert re.search(r"\bCIMBAR_HIP_TAP_ONCE_TEAR\s*=\s*33\b", header) and D.TAP_ONCE_TEAR == 33
    for name in ("cimbar_hip_set_once_tear_skip", "cimbar_hip_get_once_tear_skip"):
        assert name in D.EXPORTS and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for name in ("set_once_tear_skip", "get_once_tear_skip", "tap_once_tear"):
        assert callable(getattr(D.HipDecoder, name))
    assert (TM.LINE_DEFAULT, TM.SIDE_DEFAULT) == (750, 2)               # the defaults the header states
    assert "resolves to 750" in header and "resolves to 2" in header


def _torn_sig(mode, axis, s, o=0):
    """(P, sig, N): P all 0, N all 1, sig = P's value on the lines below s and N's from s on (o = 1: the reverse)"""
    geo = geometry.for_mode(mode)
    line, L, _ = TM.lines(mode, axis)
    P, N = np.zeros(geo.NCELLS, np.uint8), np.ones(geo.NCELLS, np.uint8)
    sig = np.where((line < s) == (o == 0), P, N).astype(np.uint8)
    return P, sig, N


def _spoil(sig, mode, axis, l, keep):
    """all but `keep` cells of line l set to a value neither neighbour has"""
    line, _, _ = TM.lines(mode, axis)
    idx = np.flatnonzero(line == l)
    out = sig.copy()
    out[idx[keep:]] = 3
    return out


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("o", [0, 1])
def test_a_clean_tear_is_found_with_its_split(axis, o):
    _, L, _ = TM.lines(MODE, axis)
    P, sig, N = _torn_sig(MODE, axis, 20, o)
    assert TM.tear(MODE, P, sig, N, axis) == (axis * 2 + o, 20, 20, L - 20)
    assert TM.tear(MODE, P, sig, N, 1 - axis) == TM.NO_TEAR           # a tear along the other axis
    assert TM.tear(MODE, P, sig, N, 2) == (axis * 2 + o, 20, 20, L - 20)
    assert TM.tear(MODE, P, P, N, axis) == TM.NO_TEAR and TM.tear(MODE, P, N, N, axis) == TM.NO_TEAR   # a whole frame of one neighbour


def test_line_permille_edge():
    _, L, width = TM.lines(MODE, 0)
    P, sig, N = _torn_sig(MODE, 0, 20)
    l, w = 10, int(width[10])
    need = -(-750 * w // 1000)                                          # the fewest cells with cnt * 1000 >= 750 * width
    assert need * 1000 >= 750 * w > (need - 1) * 1000
    assert TM.tear(MODE, P, _spoil(sig, MODE, 0, l, need), N, 0) == (0, 20, 20, L - 20)
    assert TM.tear(MODE, P, _spoil(sig, MODE, 0, l, need - 1), N, 0) == (0, 20, 19, L - 20)
    # a narrow line (it crosses the anchors) has its own width
    assert int(width[0]) == geometry.for_mode(MODE).TOP_W < w
    need0 = -(-750 * int(width[0]) // 1000)
    assert TM.tear(MODE, P, _spoil(sig, MODE, 0, 0, need0), N, 0)[2] == 20
    assert TM.tear(MODE, P, _spoil(sig, MODE, 0, 0, need0 - 1), N, 0)[2] == 19
    # the parameter itself: 1000 wants every cell, and one spoiled cell then unflags the line
    one = _spoil(sig, MODE, 0, l, w - 1)
    assert TM.tear(MODE, P, one, N, 0, line_permille=1000)[2] == 19 and TM.tear(MODE, P, sig, N, 0, line_permille=1000)[2] == 20


def test_a_line_flagged_for_both_neighbours_counts_for_neither():
    line, L, _ = TM.lines(MODE, 0)
    P, sig, N = _torn_sig(MODE, 0, 20)
    N2 = N.copy()
    N2[line == 10] = 0                                                  # both neighbours show the same on line 10
    assert TM.tear(MODE, P, sig, N2, 0) == (0, 20, 19, L - 20)
    p, q = TM.pq([8, 8, 0], [8, 0, 8], [8, 8, 8], 750)
    assert p.tolist() == [False, True, False] and q.tolist() == [False, False, True]


def _only_split(L, s):
    """min_side that leaves s as the only split of L = 2 s lines"""
    assert L == 2 * s
    return s


def test_seven_eighths_of_each_side():
    L, s = 32, 16
    ms = _only_split(L, s)
    p, q = np.zeros(L, bool), np.zeros(L, bool)
    p[:s], q[s:] = True, True
    assert TM.search(p, q, ms) == (0, s, 16, 16)
    p14, p13 = p.copy(), p.copy()
    p14[[3, 9]] = False
    p13[[3, 9, 12]] = False
    assert 8 * 14 >= 7 * s > 8 * 13
    assert TM.search(p14, q, ms) == (0, s, 14, 16) and TM.search(p13, q, ms) is None
    q14, q13 = q.copy(), q.copy()
    q14[[17, 30]] = False
    q13[[17, 30, 31]] = False
    assert TM.search(p, q14, ms) == (0, s, 16, 14) and TM.search(p, q13, ms) is None
    # the other orientation reads the same flags the other way round
    assert TM.search(q14[::-1].copy(), p[::-1].copy(), ms) == (0, s, 14, 16) and TM.search(p[::-1].copy(), q14[::-1].copy(), ms) == (1, s, 14, 16)


def test_min_side():
    L = 20
    p, q = np.zeros(L, bool), np.zeros(L, bool)
    p[:1], q[1:] = True, True
    assert TM.search(p, q, 1) == (0, 1, 1, 19)
    assert TM.search(p, q, 2) is None                                   # s = 2: one flagged line of two is below 7/8
    p[:2], q[:2] = True, False
    assert TM.search(p, q, 2) == (0, 2, 2, 18)
    p2, q2 = np.zeros(L, bool), np.zeros(L, bool)
    p2[:18], q2[18:] = True, True
    assert TM.search(p2, q2, 2) == (0, 18, 18, 2) and TM.search(p2, q2, 3) is None
    assert TM.resolve(0, 0) == (750, 2) and TM.resolve(-5, -1) == (750, 2) and TM.resolve(800, 3) == (800, 3)


def test_tie_order():
    L = 24
    p, q = np.zeros(L, bool), np.zeros(L, bool)
    p[:10], q[11:] = True, True                                         # line 10 is the one the tear crosses: flagged for neither side
    assert TM.search(p, q, 2) == (0, 10, 10, 13)                        # s = 10 and s = 11 both reach 23: the lower s
    # both orientations with the same sum (flags no capture can produce, the clause as worded): the lower o
    both = np.ones(L, bool)
    assert TM.search(both, both, 2) == (0, 2, 2, 22)
    # the larger sum wins over the lower o and the lower s
    p3, q3 = np.zeros(L, bool), np.zeros(L, bool)
    q3[:12], p3[12:] = True, True
    p3[0] = True
    q3[0] = False
    assert TM.search(p3, q3, 2) == (1, 12, 11, 12)


def test_axis_two_reports_the_axis_that_has_a_tear():
    _, L0, _ = TM.lines(MODE, 0)
    _, L1, _ = TM.lines(MODE, 1)
    P, sig, N = _torn_sig(MODE, 1, 30, 1)
    assert TM.tear(MODE, P, sig, N, 2) == (3, 30, 30, L1 - 30) and TM.tear(MODE, P, sig, N, 0) == TM.NO_TEAR
    P, sig, N = _torn_sig(MODE, 0, 30, 1)
    assert TM.tear(MODE, P, sig, N, 2) == (1, 30, 30, L0 - 30)
    # both axes admissible: the low rows show P but for their last ninth, and so do the low columns -- within 7/8 on either axis
    geo = geometry.for_mode(MODE)
    row, _, _ = TM.lines(MODE, 0)
    col, _, _ = TM.lines(MODE, 1)
    Pz, Nz = np.zeros(geo.NCELLS, np.uint8), np.ones(geo.NCELLS, np.uint8)
    sig = np.where((row < 8) | (col < 9), Pz, Nz).astype(np.uint8)     # an L of P around a block of N
    a0, a1 = TM.tear(MODE, Pz, sig, Nz, 0), TM.tear(MODE, Pz, sig, Nz, 1)
    assert a0[0] == 0 and a1[0] == 2, (a0, a1)
    assert TM.tear(MODE, Pz, sig, Nz, 2) == a0


def test_eligibility():
    members = [[0], [1], [2, 3], [4], [5]]
    runs = np.array([0, 1, 2, 2, 3, 4], np.int32)
    n = 6
    assert [TM.eligible(k, n, runs, members) for k in range(n)] == [False, True, False, False, True, False]
    runs_u = np.array([0, 1, -1, 2, 3, 4], np.int32)                   # capture 2 unusable: its neighbours are not eligible either
    members_u = [[0], [1], [3], [4], [5]]
    assert [TM.eligible(k, n, runs_u, members_u) for k in range(n)] == [False, False, False, False, True, False]


@pytest.fixture(scope="module", params=TC.MODES)
def planned(request):
    mode = request.param
    out = {}
    for name, seq in (("s1", TC.sequence1(mode)), ("s2", TC.sequence2(mode))):
        sigs, _, runs, members, _ = RM.plan(mode, seq)
        out[name] = (sigs, runs, members)
    return mode, out


def _margins(mode, axis, sigs, k, o, pix):
    geo = geometry.for_mode(mode)
    tl, sub = divmod(pix - geo.OFFSET, geo.PITCH)
    vp, vn = TM.line_permilles(mode, axis, sigs[k], sigs[k - 1]), TM.line_permilles(mode, axis, sigs[k], sigs[k + 1])
    lo, hi = (vp, vn) if o == 0 else (vn, vp)                           # lo: against the neighbour whose frame is on the low lines
    low, high = slice(0, tl), slice(tl + (1 if sub else 0), len(vp))
    same = min(lo[low].min(), hi[high].min())
    other = max(hi[low].max(), lo[high].max())
    crossed = (int(lo[tl]), int(hi[tl])) if sub else None
    return tl, sub, int(same), int(other), crossed


def test_margins_of_the_sequences(planned):
    mode, plans = planned
    cases = [("s1", 0, k, o, name) for k, (o, name) in TC.SEQ1_CANDIDATES.items()] + [("s2", 1, 3, 0, "across")]
    for seq, axis, k, o, name in cases:
        sigs = plans[seq][0]
        tl, sub, same, other, crossed = _margins(mode, axis, sigs, k, o, SC.tear_pixels(mode, axis, name)[0])
        print(mode, seq, k, name, "same-side min", same, "other-side max", other, "crossed line", crossed)
        assert same >= 900 and other <= 600
        if crossed:
            assert all(other < c < same for c in crossed)


def test_plan_of_sequence_one(planned):
    mode, plans = planned
    sigs, runs, members = plans["s1"]
    geo = geometry.for_mode(mode)
    n, full = len(sigs), geo.FULL_MASK
    assert runs.tolist() == TC.SEQ1_RUNS
    rec = TM.records(mode, sigs, runs, members, 0)
    assert TM.candidates(rec) == sorted(TC.SEQ1_CANDIDATES)
    _, L, _ = TM.lines(mode, 0)
    for k, (o, name) in TC.SEQ1_CANDIDATES.items():
        tl, sub = divmod(SC.tear_pixels(mode, 0, name)[0] - geo.OFFSET, geo.PITCH)
        assert tuple(rec[k]) == (o, tl, tl, L - tl - (1 if sub else 0)), (k, rec[k])   # the split on the torn line
    assert (TM.records(mode, sigs, runs, members, 2) == rec).all()
    assert TM.candidates(TM.records(mode, sigs, runs, members, 1)) == []
    l1 = TM.list1(members, rec)
    assert l1 == TC.SEQ1_LIST1
    masks1 = {k: full for k in l1}
    masks1[10] = full & ~1                                              # the wiped representative comes back incomplete
    l2, torn = TM.second(mode, runs, members, rec, masks1)
    assert (l2, torn) == (TC.SEQ1_LIST2, TC.SEQ1_TORN)
    R = RM
    assert TM.roles(n, runs, l1, l2, torn).tolist() == [R.SKIPPED, R.REP, R.SKIPPED, TM.TORN, R.REP, R.SKIPPED, TM.TORN, R.REP, R.FALLBACK, R.FALLBACK,
                                                        R.REP, R.FALLBACK, R.REP, R.REP, R.SKIPPED]
    # every representative complete: all three are torn and there is no list 2; none complete: nothing is withheld
    assert TM.second(mode, runs, members, rec, {k: full for k in l1}) == ([], [3, 6, 8])
    l2_none, torn_none = TM.second(mode, runs, members, rec, {k: 0 for k in l1})
    assert torn_none == [] and l2_none == [k for k in range(n) if k not in l1]
    # the setting off: the plain rule's list 1 holds the candidates
    assert sorted(l1 + TM.candidates(rec)) == [RM.representative(m) for m in members]


def test_plan_of_sequence_two(planned):
    mode, plans = planned
    sigs, runs, members = plans["s2"]
    full = geometry.for_mode(mode).FULL_MASK
    assert runs.tolist() == TC.SEQ2_RUNS
    for axis, want in TC.SEQ2_CANDIDATES_AXIS.items():
        rec = TM.records(mode, sigs, runs, members, axis)
        assert TM.candidates(rec) == want, axis
    rec = TM.records(mode, sigs, runs, members, 2)
    assert rec[3][0] == 2                                               # axis 1, orientation 0
    n = len(sigs)
    assert [TM.eligible(k, n, runs, members) for k in range(n)] == [k in (3, 8) for k in range(n)]   # the first and the last capture never
    l1 = TM.list1(members, rec)
    assert l1 == [0, 1, 5, 8, 9, 11]
    assert TM.second(mode, runs, members, rec, {k: full for k in l1}) == ([], [3])


def test_two_candidates_in_a_row_are_not_torn():
    # the guard as worded: a neighbour that is itself a candidate has not come back, so neither is torn
    runs = np.array([0, 1, 2, 3], np.int32)
    members = [[0], [1], [2], [3]]
    rec = np.array([TM.NO_TEAR, (0, 5, 5, 5), (0, 5, 5, 5), TM.NO_TEAR], np.int32)
    full = geometry.for_mode(MODE).FULL_MASK
    assert TM.list1(members, rec) == [0, 3]
    assert TM.second(MODE, runs, members, rec, {0: full, 3: full}) == ([1, 2], [])
