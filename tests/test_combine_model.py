"""CPU: the rules of multi-capture decoding (tests/combine_model.py) on hand-made arrays, and the library's new C symbols.

- grouping: runs of agreeing captures, the max_group cap, unusable captures breaking runs, the agreement threshold (a torn capture joins
  neither neighbour), groups_in taken as given and its validation
- combined cells: unanimous passthrough, the symbol vote and its tie to the lowest tile, the margin, the colour plurality and its two
  tie-breaks (smallest hash distance to the chosen symbol, then the lowest member)
"""
import ctypes
import os

import numpy as np
import pytest

from libcimbar_amd import decoder, geometry, modeb
from tests import combine_model as CM

MODE = 66                                   # the smallest grid: the cell loops of the model stay quick


def _planes(symbols_per_capture):
    """one TAP_BITPLANE-shaped byte row per capture whose cells show exactly the tiles given (no drift)"""
    geo = geometry.for_mode(MODE)
    xy = geo.cell_positions()
    tiles = np.unpackbits(modeb.TILE_HASHES.astype(">u8").view(np.uint8).reshape(16, 8), axis=1).reshape(16, 8, 8)
    out = []
    for syms in symbols_per_capture:
        bits = np.zeros((geo.IMG_H, geo.IMG_W), np.uint8)
        for i, (x, y) in enumerate(xy):
            bits[y:y + 8, x:x + 8] = tiles[syms[i]]
        out.append(np.packbits(bits.reshape(-1)))
    return np.stack(out)


def _setup(sym_rows, col_rows, plane_rows=None):
    S = np.asarray(sym_rows, np.uint8)
    C = np.asarray(col_rows, np.uint8)
    P = _planes(S if plane_rows is None else np.asarray(plane_rows, np.uint8))
    drift = np.zeros(S.shape + (2,), np.int8)
    flood = np.zeros(len(S), np.uint8)
    return P, S, C, drift, flood


def _random_cells(seed, n=None):
    geo = geometry.for_mode(MODE)
    g = np.random.default_rng(seed)
    return g.integers(0, 16, geo.NCELLS).astype(np.uint8), g.integers(0, 4, geo.NCELLS).astype(np.uint8)


def test_hash_of_a_drawn_tile_is_the_tile():
    s, _ = _random_cells(1)
    P = _planes([s])
    h = CM.cell_hashes(MODE, P[0], np.zeros((len(s), 2), np.int8), False)
    assert (h == modeb.TILE_HASHES[s]).all()


def test_unanimous_passthrough():
    s, c = _random_cells(2)
    P, S, C, drift, flood = _setup([s, s, s], [c, c, c])
    for members in ([0], [0, 1], [0, 1, 2]):
        cells, margins = CM.combine_cells(MODE, P, S, C, drift, flood, members)
        assert (cells == (c << 4) | s).all()
        assert (margins == CM.MARGIN_NONE).all()


def test_symbol_vote_majority_and_tie_to_lowest_tile():
    s, c = _random_cells(3)
    other = (s + 5) % 16
    # two members: each shows and decides its own tile -> equal scores, the lower tile wins with margin 0
    P, S, C, drift, flood = _setup([s, other], [c, c])
    cells, margins = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1])
    assert ((cells & 15) == np.minimum(s, other)).all()
    assert (margins == 0).all()
    # three members, two of them agree: the majority wins with a positive margin
    P, S, C, drift, flood = _setup([s, other, s], [c, c, c])
    cells, margins = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1, 2])
    assert ((cells & 15) == s).all()
    assert (margins > 0).all() and (margins != CM.MARGIN_NONE).all()
    # a member that decided one tile while its plane shows another is outvoted by its own hash
    P, S, C, drift, flood = _setup([s, other], [c, c], plane_rows=[s, s])
    cells, _ = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1])
    assert ((cells & 15) == s).all()


def test_colour_plurality_and_tie_breaks():
    s, c = _random_cells(4)
    c2 = (c + 1) % 4
    # plurality
    P, S, C, drift, flood = _setup([s, s, s], [c, c2, c2])
    cells, margins = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1, 2])
    assert ((cells >> 4) == c2).all() and (margins == CM.MARGIN_NONE).all()
    # a tie between equally clean members: the lowest member's colour
    P, S, C, drift, flood = _setup([s, s], [c, c2])
    cells, _ = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1])
    assert ((cells >> 4) == c).all()
    # a tie where member 0's plane shows another tile: member 1 is nearer to the symbol, its colour wins
    P, S, C, drift, flood = _setup([s, s], [c, c2], plane_rows=[(s + 3) % 16, s])
    cells, _ = CM.combine_cells(MODE, P, S, C, drift, flood, [0, 1])
    assert ((cells & 15) == s).all() and ((cells >> 4) == c2).all()


def test_drift_moves_the_hash_window():
    s, c = _random_cells(5)
    P = _planes([s])
    drift = np.zeros((1, len(s), 2), np.int8)
    drift[0, :, 0] = 1
    moved = CM.cell_hashes(MODE, P[0], drift[0], True)
    assert not (moved == modeb.TILE_HASHES[s]).all()
    assert (CM.cell_hashes(MODE, P[0], drift[0], False) == modeb.TILE_HASHES[s]).all()   # flood flag 0: drift ignored


def _frames(pattern, ncells=1000, seed=6):
    """symbols / colours of a capture stream: letters are frames, 'T' the top half of the frame before over the bottom half of the one after"""
    g = np.random.default_rng(seed)
    lib = {}
    S, C = [], []
    for k, ch in enumerate(pattern):
        if ch == "T":
            continue
        if ch not in lib:
            lib[ch] = (g.integers(0, 16, ncells), g.integers(0, 4, ncells))
    for k, ch in enumerate(pattern):
        if ch == "T":
            a, b = lib[pattern[k - 1]], lib[pattern[k + 1]]
            S.append(np.concatenate([a[0][:ncells // 2], b[0][ncells // 2:]]))
            C.append(np.concatenate([a[1][:ncells // 2], b[1][ncells // 2:]]))
        else:
            S.append(lib[ch][0]); C.append(lib[ch][1])
    return np.array(S, np.uint8), np.array(C, np.uint8)


def test_grouping_runs_torn_capture_and_cap():
    S, C = _frames("AAABBTCCC")
    assert CM.group_captures(S, C).tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 3]
    S, C = _frames("AAAAAA")
    assert CM.group_captures(S, C, max_group=4).tolist() == [0, 0, 0, 0, 1, 1]
    assert CM.group_captures(S, C, max_group=1).tolist() == [0, 1, 2, 3, 4, 5]
    assert CM.group_captures(S, C).tolist() == [0, 0, 0, 0, 1, 1]                  # default 4
    assert CM.group_captures(S, C, max_group=8).tolist() == [0] * 6
    # a few cells of noise do not break a run; a threshold above the agreement does
    S2 = S.copy()
    S2[1, :100] ^= 1
    assert CM.group_captures(S2, C, max_group=8).tolist() == [0] * 6
    assert CM.group_captures(S2, C, min_agree_permille=950, max_group=8).tolist() == [0, 1, 2, 2, 2, 2]


def test_unusable_captures_break_runs():
    S, C = _frames("AAAAA")
    assert CM.group_captures(S, C, usable=[1, 1, 0, 1, 1]).tolist() == [0, 0, -1, 1, 1]
    assert CM.group_captures(S, C, usable=[0, 1, 1, 1, 0]).tolist() == [-1, 0, 0, 0, -1]


def test_groups_in_used_as_given_and_validated():
    S, C = _frames("ABCDE")
    assert CM.group_captures(S, C, groups_in=[0, 0, -1, 1, 1]).tolist() == [0, 0, -1, 1, 1]
    assert CM.group_captures(S, C, groups_in=[0, 0, 0, 1, 1], usable=[1, 0, 1, 1, 1]).tolist() == [0, -1, 0, 1, 1]
    for bad in ([1, 1, 1, 1, 1], [0, 1, 0, 2, 2], [0, -1, 0, 1, 1], [0, 0, 0, 0, 0], [0, 2, 2, 3, 3], [-2, 0, 0, 1, 1]):
        with pytest.raises(ValueError):
            CM.group_captures(S, C, groups_in=bad)
    with pytest.raises(ValueError):
        CM.group_captures(S, C, max_group=9)
    assert CM.group_captures(S, C, groups_in=[0, 0, 0, 0, 0], max_group=5).tolist() == [0] * 5


def test_library_exports_the_combined_entry_points():
    if not os.path.exists(decoder.LIB_PATH):
        pytest.fail("libcimbar_hip.so not built: run `python -m libcimbar_amd.build` (or __graft_entry__.build())")
    lib = ctypes.CDLL(decoder.LIB_PATH)
    for name in ("cimbar_hip_decode_batch_combined", "cimbar_hip_scan_extract_decode_batch_combined_fmt"):
        assert hasattr(lib, name), name
    assert (decoder.TAP_GROUP_CELLS, decoder.TAP_GROUP_MARGIN, decoder.TAP_GROUPS) == (10, 11, 12)
