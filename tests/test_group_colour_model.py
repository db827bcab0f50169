"""CPU: the colour vote's model (tests/group_colour_model.py) on hand-made cells and on rendered two-capture groups run through the oracle.

- Hand-made: a tie in a group of two goes to the higher margin; three members at 2 : 1 where the lone member's margin exceeds the pair's sum:
  the lone member wins; all-zero margins: the lowest colour index; no dispute: 0xFFFFFFFF and no weight; the plurality restatement agrees with
  combine_model's colour half.
- Rendered pairs (group_colour_cases.pair_set, per mode): classes, positions, matrix and per-capture masks from the oracle, margins from the
  colour erasure model. Every chunk in any mask equals the payload, and over the set the vote plus the group colour retry delivers no fewer
  correct colour chunks than plurality.
- The crafted pair the GPU retry test uses: after the vote the group lacks the colour chunk, the retry recovers it with parity - 8 touched
  bytes and leaves it lost and zero with six more.
- The library exports the two new symbols and the tap ids are 15 / 16.
"""
import ctypes
import os

import numpy as np
import pytest

from libcimbar_amd import decoder, geometry
from tests import colour_erasure_model as CE
from tests import combine_model as CM
from tests import group_colour_cases as GC
from tests import group_colour_model as GM
from tests import symbol_erasure_cases as SC


def test_tie_of_two_goes_to_the_higher_margin():
    col = np.array([[1, 2, 0], [3, 1, 0]])
    mg = np.array([[100, 7, 5], [99, 8, 9]])
    c, gm, w = GM.vote(col, mg)
    assert c.tolist() == [1, 1, 0]
    assert gm.tolist() == [1, 1, GM.NONE]
    assert w.tolist() == [[101, 8, 0], [100, 9, 0]]


def test_lone_member_with_the_larger_margin_beats_a_pair():
    col = np.array([[2, 2], [2, 2], [1, 1]])
    mg = np.array([[10, 10], [20, 20], [32, 31]])
    c, gm, w = GM.vote(col, mg)
    # 33 against 11 + 21 = 32: the lone member wins by 1; 32 against 32: a tie, the lower colour index (the lone member's)
    assert c.tolist() == [1, 1] and gm.tolist() == [1, 0]
    assert w[:, 0].tolist() == [11, 21, 33]
    assert GM.plurality_colour(col).tolist() == [2, 2]


def test_all_zero_margins_lowest_colour_index():
    col = np.array([[3], [1], [2]])
    c, gm, w = GM.vote(col, np.zeros((3, 1), np.int64))
    assert c.tolist() == [1] and gm.tolist() == [0] and w[:, 0].tolist() == [1, 1, 1]
    # marg + 1: a zero-margin member still beats the colours nobody voted for
    c, gm, _ = GM.vote(np.array([[3], [3], [0]]), np.zeros((3, 1), np.int64))
    assert c.tolist() == [3] and gm.tolist() == [1]


def test_no_dispute_has_no_margin_and_no_weight():
    g = np.random.default_rng(1)
    col = np.repeat(g.integers(0, 4, (1, 500)), 3, axis=0)
    c, gm, w = GM.vote(col, g.integers(0, 390151, (3, 500)))
    assert (c == col[0]).all() and (gm == GM.NONE).all() and not w.any()
    # the largest sum fits 32 bits
    c, gm, w = GM.vote(np.array([[0]] * 7 + [[1]]), np.full((8, 1), 390150))
    assert gm.tolist() == [6 * 390151]


def test_plurality_restatement_matches_combine_model():
    from tests import test_combine_model as T
    s, c = T._random_cells(4)
    c2 = (c + 1) % 4
    for cols, planes in (([c, c2, c2], None), ([c, c2], None), ([c, c2], [(s + 3) % 16, s])):
        rows = [s] * len(cols)
        P, S, C, drift, flood = T._setup(rows, cols, plane_rows=planes)
        cells, _ = CM.combine_cells(T.MODE, P, S, C, drift, flood, list(range(len(cols))))
        H = np.stack([CM.cell_hashes(T.MODE, P[k], drift[k], False) for k in range(len(cols))])
        d = CM._popcount64(H ^ np.asarray(CM.modeb.TILE_HASHES, np.uint64)[cells & 15][None, :])
        assert (GM.plurality_colour(np.stack(cols), d) == cells >> 4).all()


def _group_inputs(mode, runs, members):
    geo = geometry.for_mode(mode)
    cells, _, disputed = SC.combine_inputs(mode, runs, members)
    cols = np.stack([runs[c]["colours"] for c in members])
    mgs = np.stack([CE.margins(CE.cell_means(runs[c]["frame"], runs[c]["positions"]), runs[c]["ccm"]) for c in members])
    for c in members:
        assert (CE.classes(CE.cell_means(runs[c]["frame"], runs[c]["positions"]), runs[c]["ccm"]) == runs[c]["colours"]).all()
    return geo, cells, disputed, cols, mgs


def _oracle(mode, caps, cc=2):
    runs = SC.oracle_run(mode, caps, cc=cc)
    for r, fr in zip(runs, caps):
        r["frame"] = fr
    return runs


def _correct(geo, mask, chunks, payload, sym_chunks):
    p = np.asarray(payload).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    n = 0
    for j in range(geo.CHUNKS_PER_FRAME):
        if (mask >> j) & 1:
            assert (chunks[j] == p[j]).all(), f"chunk {j} in the mask differs from the payload"
            n += j >= sym_chunks
        else:
            assert not chunks[j].any()
    return n


@pytest.mark.parametrize("mode", GC.MODES)
def test_rendered_pairs_vote_delivers_no_less_than_plurality(mode):
    caps, payload, groups = GC.pair_set(mode)
    runs = _oracle(mode, caps)
    symc = SC.geometry.for_mode(mode).SYM_BLOCKS // (geometry.for_mode(mode).CHUNK // geometry.for_mode(mode).RS_DATA)
    alone = plur = voted = retried = 0
    for g in range(len(payload)):
        members = [2 * g, 2 * g + 1]
        geo, cells, disputed, cols, mgs = _group_inputs(mode, runs, members)
        mm = [runs[c]["mask"] for c in members]
        mc = [runs[c]["chunks"] for c in members]
        alone += bin((mm[0] | mm[1]) >> symc).count("1")
        m0, c0, _ = GM.decode_group(geo, cells & 15, cells >> 4, None, mm, mc, disputed)
        vc, gm, _ = GM.vote(cols, mgs)
        m1, c1, _ = GM.decode_group(geo, cells & 15, vc, gm, mm, mc, disputed)
        m2, c2, _ = GM.decode_group(geo, cells & 15, vc, gm, mm, mc, disputed, colour_margin=GC.MARGIN)
        plur += _correct(geo, m0, c0, payload[g], symc)
        voted += _correct(geo, m1, c1, payload[g], symc)
        retried += _correct(geo, m2, c2, payload[g], symc)
        assert m2 & m1 == m1 and (m1 ^ m0) & ((1 << symc) - 1) == 0
    total = len(payload) * (geometry.for_mode(mode).CHUNKS_PER_FRAME - symc)
    print(f"mode {mode}: colour chunks of {total}: members alone {alone}, plurality groups {plur}, weighted groups {voted}, with retry {retried}")
    assert retried >= plur and voted >= plur


def test_crafted_pair_retry_recovers_and_overload_stays_lost():
    mode = 66
    geo = geometry.for_mode(mode)
    fr, payload = GC.K.frames(mode, 2, 71)
    true = GC.true_colours(mode, payload)
    bpc = geo.CHUNK // geo.RS_DATA
    symc = geo.SYM_BLOCKS // bpc
    e_max = geo.RS_PARITY - 8
    for k, (count, extra) in enumerate(((e_max, 6), (e_max + 6, 0))):
        a, b, touched = GC.crafted_pair(mode, fr[k], true[k], count, extra=extra)
        runs = _oracle(mode, [a, b], cc=0)          # (no matrix: washed and red cells are exact ties whatever the frame's header cells say)
        _, cells, disputed, cols, mgs = _group_inputs(mode, runs, [0, 1])
        vc, gm, w = GM.vote(cols, mgs)
        flagged = GM.byte_scores(geo, gm, GC.MARGIN)[0] > 0
        assert sorted(np.flatnonzero(flagged).tolist()) == touched
        # the members as the device reports them with the colour erasure setting on: after their own colour retry
        mm, mc = [], []
        for c, r in enumerate(runs):
            m, ch, _ = CE.retry_frame(geo, r["colours"], mgs[c], r["mask"], r["chunks"], GC.MARGIN)
            mm.append(m); mc.append(ch)
        assert not (mm[0] | mm[1]) >> symc & 1, "a member delivers the chunk alone"
        m1, c1, _ = GM.decode_group(geo, cells & 15, vc, gm, mm, mc, disputed)
        m2, c2, _ = GM.decode_group(geo, cells & 15, vc, gm, mm, mc, disputed, colour_margin=GC.MARGIN)
        assert not (m1 >> symc) & 1, "the vote alone delivers the chunk"
        _correct(geo, m2, c2, payload[k], symc)
        assert bool((m2 >> symc) & 1) == (count == e_max)


def test_library_exports_the_vote():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = ctypes.CDLL(decoder.LIB_PATH)
    for name in ("cimbar_hip_set_group_colour_vote", "cimbar_hip_get_group_colour_vote"):
        assert hasattr(lib, name), name
    assert (decoder.TAP_GROUP_COLOUR_MARGIN, decoder.TAP_GROUP_COLOUR_WEIGHTS) == (15, 16)
