"""CPU: the stream colour vote's model (tests/stream_colour_model.py) on group_colour_cases.pair_set run through the oracle, modes 68 / 67 / 66.

(a) Model equivalence: the twelve captures cut as (1,) * 12, (3, 9), (5, 7) and (2, 3, 4, 3), each member carried as per-capture results plus one
    full row of weights and nothing else, close the groups of the one-shot model over combine_model.group_captures' groups: the same members,
    masks, chunks, colours and group colour margins.
(b) The premise of the GPU test (tests/test_gpu_stream_colour.py): group_captures finds the six pairs by itself; group 4 (the largest washed
    disc) delivers no colour chunk by plurality and every chunk by the weighted vote; every chunk in any mask equals the payload.
(c) The library exports cimbar_hip_set_stream_colour_vote / cimbar_hip_get_stream_colour_vote and the new tap id is 17.
"""
import ctypes
import os

import numpy as np
import pytest

from libcimbar_amd import decoder, geometry
from tests import group_colour_cases as GC
from tests import group_colour_model as GM
from tests import stream_colour_model as SCM
from tests import symbol_erasure_cases as SC


def _sym_chunks(geo):
    return geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)


@pytest.mark.parametrize("mode", GC.MODES)
def test_cuts_close_the_one_shot_groups(mode):
    runs, _ = SCM.pair_runs(mode)
    groups, want = SCM.one_shot(mode, runs)
    assert groups.tolist() == np.repeat(np.arange(6), 2).tolist()
    for cut in SCM.CUTS:
        got = SCM.run_cut(mode, runs, cut)
        assert [g[0] for g in got] == [w[0] for w in want], cut
        for (mem, m, ch, vc, gm), (_, wm, wch, wvc, wgm) in zip(got, want):
            assert m == wm, (cut, mem, hex(m), hex(wm))
            assert (ch == wch).all() and (vc == wvc).all() and (gm == wgm).all(), (cut, mem)


@pytest.mark.parametrize("mode", GC.MODES)
def test_group_four_is_lost_by_plurality_and_whole_by_the_vote(mode):
    geo = geometry.for_mode(mode)
    runs, payload = SCM.pair_runs(mode)
    groups, voted = SCM.one_shot(mode, runs)
    assert groups.tolist() == np.repeat(np.arange(6), 2).tolist()
    symc = _sym_chunks(geo)
    pay = np.asarray(payload).reshape(len(payload), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    rows = []
    for g, (mem, m1, c1, _, _) in enumerate(voted):
        cells, _, disputed = SC.combine_inputs(mode, runs, mem)
        mm, mc = [runs[k]["mask"] for k in mem], [runs[k]["chunks"] for k in mem]
        m0, c0, _ = GM.decode_group(geo, cells & 15, cells >> 4, None, mm, mc, disputed)
        rows.append((g, [hex(x) for x in mm], hex(m0), hex(m1)))
        for mask, chunks in ((m0, c0), (m1, c1)):
            for j in range(geo.CHUNKS_PER_FRAME):
                if (mask >> j) & 1:
                    assert (chunks[j] == pay[g, j]).all(), (g, j)
        if g == 4:
            assert m0 >> symc == 0, hex(m0)
            assert m1 == geo.FULL_MASK, hex(m1)
    print(f"mode {mode}: (group, members' masks, plurality, weighted) {rows}")


def test_library_exports_the_stream_vote():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = ctypes.CDLL(decoder.LIB_PATH)
    for name in ("cimbar_hip_set_stream_colour_vote", "cimbar_hip_get_stream_colour_vote"):
        assert hasattr(lib, name), name
        assert name in decoder.EXPORTS
    assert decoder.TAP_STREAM_CARRY_WEIGHTS == 17
