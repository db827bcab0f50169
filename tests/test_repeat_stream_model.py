"""CPU: the rule of repeat-capture skipping across calls (tests/repeat_stream_model.py) on hand-made arrays, and the conditions on the inputs
that tests/test_gpu_repeat_once_stream.py relies on:

- over every split of RC.sequence into two calls, and over the split into twelve calls of one capture, the model's run boundaries are those of
  RC.SEQUENCE_RUNS -- what one plain once-call reports for the whole sequence;
- one call after reset plans what RM.plan plans;
- frame A under the 5 % wipe decodes partially (the C oracle);
- the long input (tests/repeat_stream_cases.py) has the runs it was built to have, behind a carried [A] its first run continues.
"""
import numpy as np
import pytest

from libcimbar_amd import decoder, geometry
from tests import repeat_skip_cases as RC
from tests import repeat_skip_model as RM
from tests import repeat_stream_cases as SC
from tests import repeat_stream_model as SM


def _sigs(rows, ncells=1000):
    """signatures over 1000 cells: row r is all zeros but its first `rows[r]` cells, which are 1 -- rows a and b agree in 1000 - |a - b| cells"""
    out = np.zeros((len(rows), ncells), np.uint8)
    for r, k in enumerate(rows):
        out[r, :k] = 1
    return out


class _Geo:
    """what the model reads of a geometry, for 1000 cells and 6 chunks"""
    NCELLS, FULL_MASK, CHUNKS_PER_FRAME, CHUNK = 1000, 0x3F, 6, 4


@pytest.fixture
def small(monkeypatch):
    monkeypatch.setattr(geometry, "for_mode", lambda mode: _Geo)
    return _Geo


def test_the_walk_counts_the_members_of_earlier_calls(small):
    s = _sigs([0, 10, 20, 30, 40, 50, 500])
    # one call: [0 1 2 3] [4 5] [6]
    assert SM.plan(0, SM.NOTHING, None, sigs=s).runs.tolist() == [0, 0, 0, 0, 1, 1, 2]
    # the carry inside the run of four: len 3 leaves room for one more
    c = SM.Carry(s[2], True, 3, 0, None)
    pl = SM.plan(0, c, None, sigs=s[3:])
    assert pl.continued == 1 and pl.runs.tolist() == [0, 1, 1, 2] and pl.members == [[0], [1, 2], [3]] and pl.agree[0] == 990
    # on the max_run cut: len 4 is full, capture 0 starts a run although it agrees
    c = SM.Carry(s[3], True, 4, 0, None)
    pl = SM.plan(0, c, None, sigs=s[4:])
    assert pl.continued == 0 and pl.runs.tolist() == [0, 0, 1]
    # max_run may change from call to call: a carried run of 3 is full for a call with max_run 2, and has room for a call with max_run 8
    c = SM.Carry(s[2], True, 3, 0, None)
    assert SM.plan(0, c, None, max_run=2, sigs=s[3:]).continued == 0
    assert SM.plan(0, c, None, max_run=8, sigs=s[3:]).runs.tolist() == [0, 0, 0, 1]
    # an unusable carry, an unusable capture 0, a disagreeing capture 0
    assert SM.plan(0, SM.Carry(s[2], False, 0, 0, None), None, sigs=s[3:]).continued == 0
    pl = SM.plan(0, c, None, usable=[0, 1, 1, 1], sigs=s[3:])
    assert pl.continued == 0 and pl.runs.tolist() == [-1, 0, 0, 1]
    assert SM.plan(0, c, None, sigs=s[6:]).continued == 0
    # the threshold is the plain one: 900 of 1000 joins at 900, not at 901
    c = SM.Carry(s[0], True, 1, 0, None)
    assert SM.plan(0, c, None, min_agree_permille=900, sigs=_sigs([100])).continued == 1
    assert SM.plan(0, c, None, min_agree_permille=901, sigs=_sigs([100])).continued == 0


def test_lists_fill_and_carry_honour_p(small):
    full = small.FULL_MASK
    s = _sigs([0, 10, 20, 500, 510])
    g = np.random.default_rng(5)
    row = g.integers(1, 256, (6, 4)).astype(np.uint8)
    chunks = g.integers(1, 256, (5, 6, 4)).astype(np.uint8)
    # a full P: the continued segment decodes nothing, list 1 starts at run 1
    c = SM.Carry(s[0], True, 1, full, row)
    pl = SM.plan(0, c, None, sigs=s[1:])
    assert pl.runs.tolist() == [0, 0, 1, 1] and pl.seg_p == [full, 0] and pl.list1 == [2]
    assert SM.fallback_list(0, pl, [full]) == [] and SM.fallback_list(0, pl, [full & ~1]) == [3]
    assert SM.roles(4, pl, [3]).tolist() == [0, 0, 1, 2]
    masks = np.array([0, 0, full & ~1, 1], np.uint32)
    rc, rm = SM.run_fill(0, 4, pl, c, chunks[:4], masks)
    assert rm.tolist() == [full, full, 0, 0] and (rc[0] == row).all() and (rc[1, 0] == chunks[3, 0]).all() and (rc[1, 1:] == chunks[2, 1:]).all()
    nc = SM.new_carry(4, pl, c, None, rc, rm)
    assert (nc.usable, nc.length, nc.P) == (True, 2, full) and (nc.row == rc[1]).all() and (nc.sig == s[4]).all()
    # an incomplete P: the representative is decoded; the carried row wins where P has the bit; list 2 looks at P | the representative's mask
    c = SM.Carry(s[0], True, 1, 0b000111, row)
    pl = SM.plan(0, c, None, sigs=s[1:3])
    assert pl.continued == 1 and pl.list1 == [0]
    assert SM.fallback_list(0, pl, [0b111000]) == [] and SM.fallback_list(0, pl, [0b011000]) == [1]
    masks = np.array([0b011110, 0b100001], np.uint32)
    rc, rm = SM.run_fill(0, 2, pl, c, chunks[:2], masks)
    assert rm.tolist() == [full, 0]
    assert (rc[0, :3] == row[:3]).all() and (rc[0, 3:5] == chunks[0, 3:5]).all() and (rc[0, 5] == chunks[1, 5]).all()
    nc = SM.new_carry(2, pl, c, None, rc, rm)
    assert (nc.usable, nc.length, nc.P) == (True, 3, full)
    # an unusable last capture leaves an unusable carry
    pl = SM.plan(0, c, None, usable=[1, 0], sigs=s[1:3])
    nc = SM.new_carry(2, pl, c, [1, 0], *SM.run_fill(0, 2, pl, c, chunks[:2], masks))
    assert (nc.usable, nc.length, nc.P) == (False, 0, 0)


def test_splits_of_hand_made_sequences_keep_the_plain_boundaries(small):
    g = np.random.default_rng(11)
    for trial in range(40):
        n = int(g.integers(2, 14))
        # steps of 0..40 cells between neighbours, now and then a jump: agreement 960..1000 or far below 900
        rows = np.cumsum(np.where(g.random(n) < 0.25, 300, g.integers(0, 40, n))) % 1000
        s = _sigs(rows.tolist())
        usable = g.random(n) > 0.15
        max_run = int(g.integers(1, 9))
        want = SM.plain_boundaries(0, s, usable, 900, max_run)
        for cut in range(1, n):
            assert SM.boundaries(0, s, [0, cut, n], usable, 900, max_run).tolist() == want.tolist(), (trial, cut)
        assert SM.boundaries(0, s, list(range(n + 1)), usable, 900, max_run).tolist() == want.tolist(), trial


@pytest.mark.parametrize("mode", RC.MODES)
def test_every_split_of_the_sequence_keeps_its_runs(mode):
    s = SC.sequence_sigs(mode)
    n = len(s)
    want = np.diff(np.array([-1] + RC.SEQUENCE_RUNS)) != 0
    assert SM.plain_boundaries(mode, s).tolist() == want.tolist()
    for cut in range(1, n):
        assert SM.boundaries(mode, s, [0, cut, n]).tolist() == want.tolist(), cut
    assert SM.boundaries(mode, s, list(range(n + 1))).tolist() == want.tolist()


@pytest.mark.parametrize("mode", RC.MODES)
def test_one_call_after_reset_is_the_plain_plan(mode):
    s = SC.sequence_sigs(mode)
    _, agree, runs, members, list1 = RM.plan(mode, None, sigs=s)
    pl = SM.plan(mode, SM.NOTHING, None, sigs=s)
    assert pl.continued == 0 and pl.agree[0] == 0 and pl.agree[1:].tolist() == agree.tolist()
    assert pl.runs.tolist() == runs.tolist() and pl.members == members and pl.list1 == list1 and not any(pl.seg_p)


def test_the_long_input_has_the_runs_it_was_built_to_have():
    mode, geo = SC.LONG_MODE, geometry.for_mode(SC.LONG_MODE)
    lengths, index = SC.long_layout()
    assert len(index) == SC.LONG_N > 128 and set(lengths) == {1, 2, 3, 4}
    sigs = SC.long_sigs()
    A = SC.long_pool_sigs()[0]
    carry = SM.Carry(A, True, 1, geo.FULL_MASK, np.zeros((geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8))
    pl = SM.plan(mode, carry, None, sigs=sigs)
    assert pl.continued == 1 and pl.runs.tolist() == SC.long_runs().tolist()
    assert [len(m) for m in pl.members] == list(lengths)
    # the wiped captures are the representatives of runs with other members, one in each of the first two 64-lane steps, and list 2 (should their
    # decodes be incomplete) reaches past lane 63
    reps = [RM.representative(pl.members[r]) for r in SC.LONG_WIPED_RUNS]
    assert all(index[k] >= 20 for k in reps) and (index >= 20).sum() == len(reps)
    assert reps[0] < 64 <= reps[2] < 128 and reps[1] == 63
    others = [k for r in SC.LONG_WIPED_RUNS for k in pl.members[r] if k not in reps]
    assert min(others) < 64 < max(others) and all(len(pl.members[r]) > 1 for r in SC.LONG_WIPED_RUNS)
    # the first run is skipped whole behind a full P
    assert pl.list1[0] == RM.representative(pl.members[1]) and len(pl.list1) == len(lengths) - 1


def test_the_small_wipe_delivers_some_chunks_and_not_others():
    """the precedence test's partial P: by the C oracle, frame A of mode 68 under the 5 % wipe decodes to a mask that is neither empty nor full"""
    from oracle import pyref
    W = SC.wipe5(68, RC.clean(68)[1][0])
    mask = pyref.oracle_decode(W, 0, 2, None, mode=68)[2]
    assert mask not in (0, geometry.for_mode(68).FULL_MASK), hex(mask)


def test_exports_list_the_once_stream_calls():
    for name in ("cimbar_hip_decode_batch_once_stream", "cimbar_hip_scan_extract_decode_batch_once_stream_fmt", "cimbar_hip_once_stream_reset"):
        assert name in decoder.EXPORTS
    assert decoder.TAP_REPEAT_CARRY == 30
