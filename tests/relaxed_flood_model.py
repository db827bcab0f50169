"""The relaxed flood (cimbar_hip_set_relaxed_flood) restated in numpy from its rule -- DESIGN_WIDENING.md "Relaxed flood" -- one frame at a
time, vectorised per round. What the device kernel (k_flood_rounds) is held against, cell for cell.

The rule, per frame:
  * a cell is decoded as the reference decodes it: the 10x10 window at cell_xy + drift - 1, nine 8x8 windows (cooldown 0xFE) or the first
    five of the visiting order 4,5,7,3,1,8,0,2,6, the cooldown window skipped, the first minimum over (window in that order, tile); new drift =
    drift + the window's offset clamped to +-7; calculate_cooldown;
  * a decoded cell with distance d offers (priority d, its new drift, its new cooldown) to its four adjacent cells, and to the eight horizon
    cells when the priority of the input it was decoded with is < 3, d < 3, and its input and new cooldown are both 4. Decoded cells take no offers;
  * a cell's input is the offer with the smallest (priority, offering cell) it has received; the eight seeds start with an offer of priority
    0 | 1, drift (0,0), cooldown 0xFE from "before every cell" (whose own priority counts as 0xFE in the horizon test);
  * a round: pmin = the smallest input priority among undecoded cells (none: done); T = max(threshold, pmin); all undecoded cells whose input
    priority is <= T are decoded from their inputs as they stand, then all of them make their offers.
Tables come from libcimbar_amd.geometry and the oracle (co_adjacent, co_cell_positions, co_tile_hashes)."""
import functools

import numpy as np

from libcimbar_amd import geometry
from oracle import pyref
from oracle.pyref import P

ORDER = np.array([4, 5, 7, 3, 1, 8, 0, 2, 6])
NO_OFFER = 1 << 20          # a priority no offer has
SEED_SRC = -1               # "before every cell"


@functools.lru_cache(maxsize=None)
def tables(mode):
    geo = geometry.for_mode(mode)
    L = pyref.oracle_lib(mode)
    n = geo.NCELLS
    xy = np.zeros((n, 2), np.int32)
    L.co_cell_positions(P(xy))
    adj = np.zeros((n, 4), np.int32)
    for i in range(n):
        L.co_adjacent(i, P(adj[i]))
    # FloodDecodePositions::update's offer list: right, left, bottom, top; then two cells further right and left (if the cell has both a right
    # and a left neighbour), then two further up and down (if it has both a top and a bottom one)
    t = np.full((n, 12), -1, np.int32)
    t[:, :4] = adj

    def step(cells, direction):
        return np.where(cells >= 0, adj[np.maximum(cells, 0), direction], -1)
    rr, ll, dd, uu = adj[:, 0], adj[:, 1], adj[:, 2], adj[:, 3]
    h = (rr >= 0) & (ll >= 0)
    v = (uu >= 0) & (dd >= 0)
    t[:, 4] = np.where(h, step(rr, 0), -1); t[:, 5] = step(t[:, 4], 0)
    t[:, 6] = np.where(h, step(ll, 1), -1); t[:, 7] = step(t[:, 6], 1)
    t[:, 8] = np.where(v, step(uu, 3), -1); t[:, 9] = step(t[:, 8], 3)
    t[:, 10] = np.where(v, step(dd, 2), -1); t[:, 11] = step(t[:, 10], 2)
    hashes = np.zeros(16, np.uint64)
    L.co_tile_hashes(P(hashes))
    # bit 63 of a hash = the top-left pixel of the 8x8 tile, row-major
    tiles = ((hashes[:, None] >> np.arange(63, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int32)      # (16, 64)
    last = n - 1
    seeds = [(0, 0), (geo.TOP_W - 1, 0), (last, 0), (last - (geo.TOP_W - 1), 0), (geo.TOP_CELLS, 1), (geo.TOP_CELLS + geo.DIM_X - 1, 1),
             (last - geo.TOP_CELLS, 1), (last - (geo.TOP_CELLS + geo.DIM_X - 1), 1)]
    return geo, xy, t, tiles, seeds


def calculate_cooldown(previous, idx):
    """CellDrift::calculate_cooldown, elementwise"""
    out = np.where(idx % 2 == 0, 0xFF, np.where(((previous ^ idx) & 0xFF) == 6, 0xFF, idx))
    return np.where(idx == 4, 4, out)


def decode_cells(bits, xy, tiles, cells, dx, dy, cooldown):
    """-> (symbol, window, distance) of each cell decoded at drift (dx, dy) with `cooldown`"""
    m = len(cells)
    x0 = xy[cells, 0] + dx - 1
    y0 = xy[cells, 1] + dy - 1
    r = np.arange(10)
    win = bits[(y0[:, None] + r[None, :])[:, :, None], (x0[:, None] + r[None, :])[:, None, :]].astype(np.int32)        # (m, 10, 10)
    sub = np.stack([win[:, w // 3:w // 3 + 8, w % 3:w % 3 + 8].reshape(m, 64) for w in ORDER], 1)                      # (m, 9, 64) in visiting order
    dist = sub @ (1 - tiles.T) + (1 - sub) @ tiles.T                                                                   # (m, 9, 16) Hamming distances
    k = np.arange(9)
    allowed = (k[None, :] < np.where(cooldown == 0xFE, 9, 5)[:, None]) & ~((ORDER[None, :] == cooldown[:, None]) & (ORDER[None, :] != 4))
    key = dist * 256 + k[None, :, None] * 16 + np.arange(16)[None, None, :]
    key = np.where(allowed[:, :, None], key, 1 << 30).reshape(m, -1)
    best = key.min(1)
    return best & 15, ORDER[(best >> 4) & 15], best >> 8


def relaxed_flood(bitplane, mode=68, threshold=12, rng=None):
    """bitplane: one frame's TAP_BITPLANE bytes. Returns (symbols u8 [cells], drift i8 [cells, 2], rounds, distances [cells]); a cell no offer
    ever reached keeps distance -1. rng: the order in which a round's cells make their offers is permuted with it (it must not matter)."""
    geo, xy, targets, tiles, seeds = tables(mode)
    n = geo.NCELLS
    bits = np.unpackbits(np.ascontiguousarray(bitplane, dtype=np.uint8).reshape(-1))[:geo.IMG_W * geo.IMG_H].reshape(geo.IMG_H, geo.IMG_W)
    prio = np.full(n, NO_OFFER, np.int64)
    src = np.full(n, n, np.int64)
    in_dx = np.zeros(n, np.int64); in_dy = np.zeros(n, np.int64); in_cool = np.full(n, 0xFE, np.int64)
    for cell, p in seeds:
        prio[cell] = p
        src[cell] = SEED_SRC
    decoded = np.zeros(n, bool)
    sym = np.zeros(n, np.uint8)
    drift = np.zeros((n, 2), np.int8)
    dists = np.full(n, -1, np.int32)
    rounds = 0
    while True:
        open_ = ~decoded & (prio < NO_OFFER)
        if not open_.any():
            break
        T = max(int(threshold), int(prio[open_].min()))
        mem = np.flatnonzero(open_ & (prio <= T))
        rounds += 1
        dx, dy, cool = in_dx[mem], in_dy[mem], in_cool[mem]
        s, w, d = decode_cells(bits, xy, tiles, mem, dx, dy, cool)
        bx, by = w % 3 - 1, w // 3 - 1
        sym[mem] = s
        drift[mem, 0] = dx + bx
        drift[mem, 1] = dy + by
        dists[mem] = d
        decoded[mem] = True
        ndx, ndy = np.clip(dx + bx, -7, 7), np.clip(dy + by, -7, 7)
        ncool = calculate_cooldown(cool, w)
        din = np.where(src[mem] == SEED_SRC, 0xFE, prio[mem])
        far = (din < 3) & (d < 3) & (cool == 4) & (ncool == 4)
        # every (offering cell, target) pair of the round
        who = np.repeat(np.arange(len(mem)), 12)
        tg = targets[mem].reshape(-1)
        ok = (tg >= 0) & (far[who] | (np.tile(np.arange(12), len(mem)) < 4))
        ok &= ~decoded[np.maximum(tg, 0)]
        who, tg = who[ok], tg[ok]
        if rng is not None:
            o = rng.permutation(len(who))
            who, tg = who[o], tg[o]
        # one offer after the other: it replaces the target's input iff its (priority, offering cell) is smaller
        for a, c in zip(who, tg):
            i = mem[a]
            if (d[a], i) < (prio[c], src[c]):
                prio[c], src[c], in_dx[c], in_dy[c], in_cool[c] = d[a], i, ndx[a], ndy[a], ncool[a]
        if rounds > n:
            raise AssertionError("a round decoded nothing")
    return sym, drift, rounds, dists


def table_cases(clean):
    """The distortions of the table in DESIGN_WIDENING.md "Relaxed flood", of frames 0 and 1 of `clean` (mode 68, clean_frames(synth, 2, seed=123)):
    [(name, frame index, frame)]"""
    from tests import frames as F
    cases = []
    for i in range(2):
        c = clean[i]
        cases += [("shift(2,1)", i, F.shift(c, 2, 1)), ("shift(-3,3)", i, F.shift(c, -3, 3)), ("add_noise(120)", i, F.add_noise(c, 120, i)),
                  ("rescale(6)", i, F.rescale(c, 6)), ("rescale(10)", i, F.rescale(c, 10)),
                  ("add_noise(shift(1,-2), 60)", i, F.add_noise(F.shift(c, 1, -2), 60, i)),
                  ("add_noise(rescale(5), 60)", i, F.add_noise(F.rescale(c, 5), 60, i)),
                  ("wipe 200x500", i, F.blank_region(F.shift(c, 1, 1), 300, 500, 200, 700, value=128)),
                  ("tear (two shifts)", i, np.concatenate([F.shift(c, 1, 0)[:500], F.shift(c, 0, 1)[500:]], 0))]
    return cases


def exact_flood(frame, mode=68):
    """the oracle's bit plane of `frame` and the symbols of the reference's priority flood on it (co_symbol_pass)"""
    geo = geometry.for_mode(mode)
    L = pyref.oracle_lib(mode)
    plane = np.zeros(geo.IMG_W * geo.IMG_H // 8, np.uint8)
    L.co_threshold_bitplane(P(np.ascontiguousarray(frame)), geo.IMG_W, geo.IMG_H, 0, P(plane))
    visit = np.zeros(4 * geo.NCELLS, np.int32)
    n = L.co_symbol_pass(P(plane), P(visit), None)
    v = visit.reshape(-1, 4)[:n]
    sym = np.zeros(geo.NCELLS, np.uint8)
    sym[v[:, 0]] = v[:, 3]
    return plane, sym
