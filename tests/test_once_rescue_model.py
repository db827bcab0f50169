"""CPU: the rule of the run rescue (tests/once_rescue_model.py) on hand-made masks, the signature margins its GPU inputs rely on in modes
68 / 67 / 66, and the two symbols the feature adds to the library.

The margins are conditions on the inputs, not tolerances of the device code. With min_agree_permille = 500:
- the two members of a disjoint-disc pair agree in at least 800 permille of the ink signatures (measured 823 .. 880 over the modes): one run;
- neighbours in a three-band triple agree in at least 550 (measured 575 .. 595): one run;
- captures of two different frames, damaged or not, agree in at most 300 (clean frames: 254 .. 260): two runs.
All of the first two stay below 900, so the default joins none of them.
"""
import numpy as np
import pytest

from libcimbar_amd import decoder, geometry
from tests import once_rescue_model as OM
from tests import repeat_skip_model as RM


def test_which_runs_are_tried():
    full = geometry.for_mode(66).FULL_MASK
    #          a run of one | the representative (capture 1) complete | pass 2 completes it | stays incomplete (rep = the middle, 9)
    members = [[0], [1, 2], [3, 4, 5], [8, 9, 10]]
    masks = np.zeros(11, np.uint32)
    masks[0] = 0b000011
    masks[1], masks[2] = full, 0                       # capture 2 was skipped
    masks[3], masks[4], masks[5] = 0b110000, 0b000111, 0b001000
    masks[8], masks[9], masks[10] = 0b000001, 0b000010, 0b000100
    assert OM.tried(66, members, masks) == [False, False, False, True]
    # a pair whose representative is incomplete and whose other member completes it alone
    assert OM.tried(66, [[0, 1]], np.array([0b1, full], np.uint32)) == [False]
    assert OM.tried(66, [[0, 1]], np.array([0b1, 0b10], np.uint32)) == [True]
    # the tap word: what the row has beyond the members' OR; -1 where nothing was tried and past the run count
    rows = np.array([0b000011, full, full, 0b010111], np.uint32)
    assert OM.tap_words(66, 11, members, masks, rows).tolist() == [-1, -1, -1, 0b010000] + [-1] * 7
    rows[3] = 0b000111                                 # tried, nothing gained: 0, not -1
    assert OM.tap_words(66, 11, members, masks, rows)[3] == 0


def test_row_composition():
    geo = geometry.for_mode(66)
    g = np.random.default_rng(5)
    chunks = g.integers(0, 256, (3, geo.CHUNKS_PER_FRAME, geo.CHUNK)).astype(np.uint8)
    cchunks = g.integers(0, 256, (geo.CHUNKS_PER_FRAME, geo.CHUNK)).astype(np.uint8)
    masks = np.array([0b000110, 0b000011, 0b001010], np.uint32)
    # the combined decode has chunks 1 and 4, the retry added chunk 5; member order is capture order whoever the representative is
    row, mask = OM.compose_row(66, [0, 1, 2], chunks, masks, cchunks, 0b010010, 0b100000)
    assert mask == 0b111111
    assert (row[1] == cchunks[1]).all() and (row[4] == cchunks[4]).all() and (row[5] == cchunks[5]).all()
    assert (row[0] == chunks[1, 0]).all() and (row[2] == chunks[0, 2]).all() and (row[3] == chunks[2, 3]).all()
    # nothing from the group decode: the lowest-index member that has the chunk, zeros for what nobody has
    row, mask = OM.compose_row(66, [0, 1, 2], chunks, masks, cchunks, 0)
    assert mask == 0b001111 and (row[1] == chunks[0, 1]).all() and not row[4:].any()
    # rows of runs that are not tried are the plain fill's; a tried run's row is the group's
    members = [[0, 1], [2]]
    gch = g.integers(0, 256, (3, geo.CHUNKS_PER_FRAME, geo.CHUNK)).astype(np.uint8)
    gm = np.array([geo.FULL_MASK, 0b1, 0], np.uint32)
    rc, rm = OM.run_rows(66, 3, members, chunks, masks, gch, gm)
    want_c, want_m = RM.run_fill(66, 3, members, chunks, masks)
    assert OM.tried(66, members, masks) == [True, False]
    assert rm.tolist() == [geo.FULL_MASK, int(want_m[1]), 0] and (rc[0] == gch[0]).all() and (rc[1:] == want_c[1:]).all()
    # a superset of the plain fill's mask whenever the group row holds the members' chunks
    assert all(int(a) & int(b) == int(b) for a, b in zip(rm, want_m))


@pytest.mark.parametrize("mode", OM.MODES)
def test_margins_of_the_gpu_inputs(mode):
    caps, _ = OM.rendered(mode)
    b = OM.bands(mode)
    table = {"pair": [RM.permille(mode, caps[3 * k + 1], caps[3 * k + 2]) for k in range(3)],
             "bands": [RM.permille(mode, b[0], b[1]), RM.permille(mode, b[1], b[2])],
             "frames": [RM.permille(mode, caps[0], caps[3]), RM.permille(mode, caps[3], caps[6]), RM.permille(mode, caps[0], caps[6])]}
    print("once-rescue agreement, mode", mode, table)
    assert all(800 <= p < 900 for p in table["pair"]), table
    assert all(550 <= p < 900 for p in table["bands"]), table
    assert all(p <= 300 for p in table["frames"]), table
    # the sequence and the 70 pairs fall into the runs they were built as at 500, and into single captures at the default
    seq = OM.sequence(mode)
    _, agree, runs, members, list1 = RM.plan(mode, seq, None, OM.MIN_AGREE, 0)
    assert runs.tolist() == OM.SEQUENCE_RUNS and list1 == OM.SEQUENCE_LIST1
    ncells = geometry.for_mode(mode).NCELLS
    breaks = [int(a) * 1000 // ncells for k, a in enumerate(agree) if runs[k] != runs[k + 1]]
    assert max(breaks) <= 300, breaks
    assert RM.plan(mode, seq[[0, 1, 4, 5, 6]], None, 0, 0)[2].tolist() == list(range(5))
    if mode == 66:
        frames, _ = OM.pairs(mode, 70)
        sig3 = RM.signatures(mode, frames[:6])         # the 140 captures are these six in turn
        runs = RM.plan(mode, frames, None, OM.MIN_AGREE, 0, sigs=sig3[np.arange(140) % 6])[2]
        assert runs.tolist() == [k // 2 for k in range(140)]


def test_the_library_exports_the_setting():
    assert "cimbar_hip_set_once_rescue" in decoder.EXPORTS and "cimbar_hip_get_once_rescue" in decoder.EXPORTS
    assert (decoder.TAP_ONCE_RESCUE, decoder.TAP_ONCE_RESCUE_CELLS) == (31, 32)
    lib = decoder.load_library()
    assert hasattr(lib, "cimbar_hip_set_once_rescue") and hasattr(lib, "cimbar_hip_get_once_rescue")
