"""Phase 2 of the parallel symbol pass (k_symbols) restated in numpy for one mode, from its rule -- DESIGN.md "K2 `k_symbols` -- parallel symbol
pass + proof obligation" -- with nothing taken from the kernel side. Geometry comes from libcimbar_amd.geometry, the 16 tile hashes and the cell
positions from the oracle (co_tile_hashes, co_cell_positions).

The rule, per frame, on a bit plane (H, W) of 0/1:
  * a cell at (x, y) has a 10x10 window whose top-left pixel is (x - 1, y - 1), and in it nine 8x8 windows: window w is the cell's own block
    shifted by (w % 3 - 1, w // 3 - 1); window 4 is the centre. A window's hash has its top-left pixel in bit 63, row-major;
  * a window's key is distance << 4 | tile, the smallest over the 16 tiles: the first minimum wins (CimbDecoder.cpp:111-131);
  * the parallel symbol of a cell is the tile of its centre key, dc its distance;
  * a cell violates the fast-path condition when dc != 0 and some other window's distance is strictly below dc: the side windows 5, 7, 3, 1 for
    an ordinary cell, those and the corner windows 8, 0, 2, 6 for the eight flood seeds (FloodDecodePositions.cpp:27-41), which the reference may
    decode in nine-window mode;
  * the frame is flagged when any cell violates. The theorem: the reference's flood visits every cell of an unflagged frame undrifted, with the
    parallel symbol, whatever its heap order.

`STRICT` and `SEEDS_LOOK_AT_CORNERS` are the two halves of the rule that tests/test_fast_path_model.py mutates."""
import functools
from dataclasses import dataclass

import numpy as np

from libcimbar_amd import geometry
from oracle import pyref
from oracle.pyref import P

SIDES = (5, 7, 3, 1)
CORNERS = (8, 0, 2, 6)
STRICT = True                    # False: `<=` in place of `<` (a mutation: sets 1 and 4 must then fail)
SEEDS_LOOK_AT_CORNERS = True     # False: the seeds look at their side windows only (a mutation: set 4's seed frames must then fail)
QUEUE_ROWS = 8                   # cell rows per wavefront of the device's pass: only the queue order below depends on it


@dataclass(frozen=True)
class Tables:
    geo: object
    xy: np.ndarray          # (NCELLS, 2) top-left pixel of every cell
    row: np.ndarray         # (NCELLS,) grid row and column of every cell
    col: np.ndarray
    tiles: np.ndarray       # (16, 64) 0/1, the tiles' pixels row-major
    hashes: np.ndarray      # (16,) uint64
    seeds: np.ndarray       # (8,) cell indices
    is_seed: np.ndarray     # (NCELLS,) bool


@functools.lru_cache(maxsize=None)
def tables(mode):
    geo = geometry.for_mode(mode)
    L = pyref.oracle_lib(mode)
    n = geo.NCELLS
    xy = np.zeros((n, 2), np.int32)
    L.co_cell_positions(P(xy))
    hashes = np.zeros(16, np.uint64)
    L.co_tile_hashes(P(hashes))
    assert len(set(hashes.tolist())) == 16
    tiles = ((hashes[:, None] >> np.arange(63, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int32)
    last, small_row, between = n - 1, geo.TOP_W, geo.TOP_CELLS
    seeds = np.array([0, small_row - 1, last, last - (small_row - 1), between, between + geo.DIM_X - 1, last - between,
                      last - (between + geo.DIM_X - 1)], np.int64)
    is_seed = np.zeros(n, bool)
    is_seed[seeds] = True
    row = (xy[:, 1] - geo.OFFSET) // geo.PITCH
    col = (xy[:, 0] - geo.OFFSET) // geo.PITCH
    assert ((xy[:, 0] - geo.OFFSET) % geo.PITCH == 0).all() and ((xy[:, 1] - geo.OFFSET) % geo.PITCH == 0).all()
    return Tables(geo, xy, row, col, tiles, hashes, seeds, is_seed)


def unpack_plane(packed, mode):
    """co_threshold_bitplane's bytes (MSB = leftmost pixel) -> (H, W) uint8 of 0/1"""
    geo = geometry.for_mode(mode)
    return np.unpackbits(np.asarray(packed, np.uint8).reshape(geo.IMG_H, geo.IMG_W // 8), axis=1)


def cell_windows(plane, mode, cells=None):
    """(n, 10, 10) 0/1: the 10x10 windows of `cells` (all of them by default)"""
    T = tables(mode)
    xy = T.xy if cells is None else T.xy[np.asarray(cells)]
    k = np.arange(10)
    return plane[(xy[:, 1, None, None] - 1) + k[None, :, None], (xy[:, 0, None, None] - 1) + k[None, None, :]]


def window_bits(win):
    """(n, 10, 10) -> (n, 9, 64): the nine 8x8 windows' pixels, row-major"""
    return np.stack([win[:, w // 3:w // 3 + 8, w % 3:w % 3 + 8].reshape(len(win), 64) for w in range(9)], 1)


def window_hashes(win):
    """(n, 10, 10) -> (n, 9) uint64, the top-left pixel in bit 63"""
    b = np.packbits(window_bits(win).astype(np.uint8), axis=2)          # (n, 9, 8), most significant byte first
    return np.ascontiguousarray(b).view(">u8")[..., 0].astype(np.uint64)


def window_distances(win, mode):
    """(n, 10, 10) -> (n, 9, 16): Hamming distance of every window to every tile"""
    t = tables(mode).tiles
    bits = window_bits(win).astype(np.int32)
    # popcount(a ^ t) = sum a + sum t - 2 a.t
    return bits.sum(2)[..., None] + t.sum(1)[None, None, :] - 2 * (bits @ t.T)


def window_keys(win, mode):
    """(n, 10, 10) -> (n, 9): distance << 4 | tile, the first minimum over the tiles"""
    d = window_distances(win, mode)
    return ((d << 4) | np.arange(16)[None, None, :]).min(2)


@dataclass
class Result:
    keys: np.ndarray        # (n, 9)
    symbols: np.ndarray     # (n,) uint8: the parallel symbols
    dc: np.ndarray          # (n,) centre distance
    side: np.ndarray        # (n,) the smallest distance over the four side windows
    corner: np.ndarray      # (n,) ... over the four corner windows
    other: np.ndarray       # (n,) ... over the windows the cell's rule looks at
    ties: np.ndarray        # (n,) tiles at the centre's minimum distance
    violates: np.ndarray    # (n,) bool
    flag: int

    def describe(self, T, i):
        return f"cell {i} = (row {T.row[i]}, column {T.col[i]}){' [seed]' if T.is_seed[i] else ''}: dc {self.dc[i]}, side {self.side[i]}, corner {self.corner[i]}"


def classify(win, is_seed, mode):
    """the rule on (n, 10, 10) windows; is_seed (n,) bool"""
    d = window_distances(win, mode)
    keys = ((d << 4) | np.arange(16)[None, None, :]).min(2)
    dist = keys >> 4
    dc = dist[:, 4]
    side = dist[:, list(SIDES)].min(1)
    corner = dist[:, list(CORNERS)].min(1)
    other = np.where(is_seed & SEEDS_LOOK_AT_CORNERS, np.minimum(side, corner), side)
    violates = (dc != 0) & ((other < dc) if STRICT else (other <= dc))
    ties = (d[:, 4, :] == dc[:, None]).sum(1)
    return Result(keys, (keys[:, 4] & 15).astype(np.uint8), dc, side, corner, other, ties, violates, int(violates.any()))


def evaluate(plane, mode):
    """the rule on a whole plane (H, W) of 0/1"""
    return classify(cell_windows(plane, mode), tables(mode).is_seed, mode)


def class_counts(res, mode):
    """what a frame holds of the cells the strict comparison, the seed rule and the first-minimum choice decide"""
    T = tables(mode)
    inexact = res.dc != 0
    return {"inexact": int(inexact.sum()),
            "side_ties": int((inexact & (res.side == res.dc)).sum()),
            "corner_better": int((inexact & ~T.is_seed & (res.corner < res.dc)).sum()),
            "tile_ties": int((res.ties >= 2).sum()),
            "violating": int(res.violates.sum())}


def queue_slots(res, mode):
    """(strip, slot) per cell: the wavefront that owns the cell (QUEUE_ROWS cell rows each) and the cell's place in that wavefront's queue of
    inexact cells, -1 for an exact cell. The queue is filled a pair of cell rows at a time; within a pair, by the cell's rank among the cells
    whose block starts in the same 32-bit plane word, then by lane = 32 * (row & 1) + word. A wavefront walks its queue 64 slots at a time."""
    T = tables(mode)
    geo = T.geo
    x0 = T.xy[:, 0]
    word = x0 >> 5
    first_col = np.where(word == 0, 0, -((geo.OFFSET - 32 * word) // geo.PITCH))       # the first column whose block starts in this word
    rank = T.col - first_col
    assert (rank >= 0).all() and (rank < 4).all()
    strip = T.row // QUEUE_ROWS
    order = np.lexsort((word, T.row & 1, rank, (T.row % QUEUE_ROWS) // 2, strip))
    slot = np.full(geo.NCELLS, -1, np.int64)
    queued = res.dc[order] != 0
    s = strip[order]
    pos = np.cumsum(queued) - 1
    start = np.zeros(s.max() + 1, np.int64)                  # queued cells in front of each strip
    np.add.at(start, s[queued], 1)
    start = np.concatenate([[0], np.cumsum(start)[:-1]])
    slot[order[queued]] = (pos - start[s])[queued]
    return strip, slot
