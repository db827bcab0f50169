"""Frames on the line between the parallel symbol pass's two outcomes (k_symbols: "this frame is the reference's result as it stands" /
"flag it for the flood kernels"), built deterministically per mode and shared by tests/test_fast_path_model.py and tests/test_gpu_fast_path.py.

Every case is a gray frame 255 * plan (the same value on the three channels) of a planned bit plane. Without the sharpen pass the 5x5 mean
threshold gives the plan back except where a set bit sits in a solid 5x5 block of ones, so every statement about a case is made on
co_threshold_bitplane of its frame (`plane`), never on the plan; the builders below loop until that plane says what the case is meant to say.

A plan is a clean frame's plane with bits flipped inside the cells' own 8x8 blocks only (the 1-pixel gaps between cells are never touched).

Sets (tests/fast_path_model.py names the rule and the counts):
  1 boundary      four frames with 12, 16, 20 and 24 flips per cell; the cells that violate the condition are put back to their clean bits until
                  none does: unflagged, with thousands of inexact cells, side windows that tie the centre, corner windows that beat it
  2 queue         1 flip in every cell, and 4: every cell inexact, none violating: the device's per-wavefront queue at its capacity
  3 one cell      boundary frame 0 with one cell's flips drawn again until its best other window is exactly one closer than its centre:
                  flagged, by that cell alone; one frame per location (LOCATIONS)
  4 seeds         per seed a frame in which that seed has a corner window strictly closer than the centre and no side window closer (flagged),
                  and one frame in which the eight seeds' non-seed neighbours have that and the seeds are clean (unflagged)
  5 split         the frames of sets 1 to 4 repeated cyclically to 160 frames: the batch size at which the chain runs as two half-batches"""
import functools

import numpy as np

from libcimbar_amd import framegen, geometry
from oracle import pyref
from oracle.pyref import P
from tests import fast_path_model as M
from tests import frames as F

MODES = [68, 67, 66, 4, 8]
BOUNDARY_FLIPS = (12, 16, 20, 24)
QUEUE_FLIPS = (1, 4)
SPLIT_FRAMES = 160
FLOORS = {"side_ties": 500, "corner_better": 500, "tile_ties": 50}     # on the 20-flip boundary frame, in every mode
SEED = 20250               # of everything below; a seed that misses a floor or a condition is changed here, the floor and the condition stay


class Case:
    def __init__(self, mode, set_no, name, plan, flagged, cells=()):
        self.mode, self.set, self.name, self.flagged, self.cells = mode, set_no, name, flagged, tuple(int(c) for c in cells)
        self._plan = np.packbits(plan, axis=1)
        self.packed = np.packbits(threshold(self.frame, mode), axis=1).reshape(-1)      # the plane as co_threshold_bitplane and TAP_BITPLANE give it

    @property
    def frame(self):
        return frame_of(np.unpackbits(self._plan, axis=1))

    @property
    def plane(self):
        return M.unpack_plane(self.packed, self.mode)

    @functools.cached_property
    def result(self):
        return M.evaluate(self.plane, self.mode)

    def __repr__(self):
        return f"mode {self.mode} set {self.set} case {self.name}"


def frame_of(plan):
    return np.ascontiguousarray(np.repeat((plan * 255).astype(np.uint8)[:, :, None], 3, 2))


def threshold(frame, mode):
    """co_threshold_bitplane without the sharpen pass, as (H, W) 0/1"""
    geo = geometry.for_mode(mode)
    out = np.zeros(geo.IMG_W * geo.IMG_H // 8, np.uint8)
    pyref.oracle_lib(mode).co_threshold_bitplane(P(np.ascontiguousarray(frame)), geo.IMG_W, geo.IMG_H, 0, P(out))
    return M.unpack_plane(out, mode)


def threshold_patch(patch):
    """the same threshold on (n, h, w) 0/1 patches of a 255 * plan frame, for their inner (h - 4, w - 4): a set bit stays unless its 5x5 block is
    all ones (255 > mean fails only there)"""
    h, w = patch.shape[1] - 4, patch.shape[2] - 4
    solid = np.ones((len(patch), h, w), bool)
    for dy in range(5):
        for dx in range(5):
            solid &= patch[:, dy:dy + h, dx:dx + w] != 0
    return (patch[:, 2:2 + h, 2:2 + w] != 0) & ~solid


@functools.lru_cache(maxsize=None)
def clean_plan(mode):
    """a clean frame's plane"""
    synth = framegen.FrameSynth("cpu", mode)
    _, frames = F.clean_frames(synth, 1, seed=SEED + mode)
    return threshold(frames[0], mode)


def block_index(mode, cells=None):
    """(n, 64) row and column indices of the cells' own 8x8 blocks, row-major"""
    T = M.tables(mode)
    xy = T.xy if cells is None else T.xy[np.asarray(cells)]
    k = np.arange(64)
    return xy[:, 1, None] + k[None, :] // 8, xy[:, 0, None] + k[None, :] % 8


def flipped(mode, flips, rng):
    """the clean plan with exactly `flips` bits flipped in every cell's block"""
    plan = clean_plan(mode).copy()
    n = M.tables(mode).geo.NCELLS
    which = np.argsort(rng.random((n, 64)), axis=1)[:, :flips]
    ys, xs = block_index(mode)
    r = np.arange(n)[:, None]
    plan[ys[r, which], xs[r, which]] ^= 1
    return plan


def restore(plan, mode, cells):
    ys, xs = block_index(mode, cells)
    plan[ys, xs] = clean_plan(mode)[ys, xs]


def repaired(mode, plan, keep=()):
    """put the violating cells (but `keep`) back to their clean bits until the thresholded plane holds none"""
    keep = np.asarray(keep, np.int64)
    for _ in range(12):
        res = M.evaluate(threshold(frame_of(plan), mode), mode)
        bad = np.setdiff1d(np.flatnonzero(res.violates), keep)
        if bad.size == 0:
            return plan
        restore(plan, mode, bad)
    raise AssertionError(f"mode {mode}: the repair does not settle")


def redraw(mode, plan, cells, accept, rng, flips, name):
    """draw the flips of `cells` again (one cell at a time, the others as they stand) until `accept(result of the cell)` holds for each on the
    thresholded plane and no other cell violates. Candidates are screened on the cell's own 14x14 patch first, a few thousand at a time."""
    T = M.tables(mode)
    clean = clean_plan(mode)
    plan = plan.copy()
    for c in cells:
        x, y = int(T.xy[c, 0]), int(T.xy[c, 1])
        seed_c = np.array([T.is_seed[c]])
        done = False
        for attempt in range(40):
            nf = flips + attempt % 17                      # more flips bring the centre distance up to where other windows can beat it
            k = 4096
            patch = np.repeat(plan[None, y - 3:y + 11, x - 3:x + 11], k, 0)
            block = np.repeat(clean[None, y:y + 8, x:x + 8].reshape(1, 64), k, 0)
            which = np.argsort(rng.random((k, 64)), axis=1)[:, :nf]
            block[np.arange(k)[:, None], which] ^= 1
            patch[:, 3:11, 3:11] = block.reshape(k, 8, 8)
            res = M.classify(threshold_patch(patch).astype(np.uint8), np.repeat(seed_c, k), mode)
            for j in np.flatnonzero(accept(res))[:8]:
                trial = plan.copy()
                trial[y:y + 8, x:x + 8] = block[j].reshape(8, 8)
                full = M.evaluate(threshold(frame_of(trial), mode), mode)
                one = M.Result(*(getattr(full, f)[c:c + 1] for f in ("keys", "symbols", "dc", "side", "corner", "other", "ties", "violates")), 0)
                others = full.violates.copy()
                others[list(cells)] = False
                if accept(one)[0] and not others.any():
                    plan, done = trial, True
                    break
            if done:
                break
        assert done, f"mode {mode} {name}: no draw found for cell {c}"
    return plan


# ------------------------------------------------------------------------------------------------ the sets
@functools.lru_cache(maxsize=None)
def boundary(mode):
    out = []
    for k, flips in enumerate(BOUNDARY_FLIPS):
        rng = np.random.default_rng([SEED, mode, 1, flips])
        out.append(Case(mode, 1, f"boundary-{flips}", repaired(mode, flipped(mode, flips, rng)), False))
    return out


@functools.lru_cache(maxsize=None)
def queue_stress(mode):
    """exactly `flips` flips in every cell and nothing put back, so a draw in which some cell violates (about one in five with 4 flips) is
    drawn again: the first draw, in a fixed order, that leaves every cell inexact and none violating"""
    out = []
    for flips in QUEUE_FLIPS:
        for draw in range(16):
            case = Case(mode, 2, f"queue-{flips}", flipped(mode, flips, np.random.default_rng([SEED, mode, 2, flips, draw])), False)
            if not case.result.flag and (case.result.dc != 0).all():
                break
        out.append(case)      # (a last draw that still misses is left for tests/test_fast_path_model.py to report)
    return out


def base_plan(mode):
    """the plan sets 3 and 4 start from: the plane of boundary frame 0 (a plane is its own plan: thresholding it again changes nothing that
    thresholding did not change already -- and the builders check their results on the thresholded plane anyway)"""
    return boundary(mode)[0].plane.copy()


def locations(mode):
    """name -> cell of set 3, chosen on boundary frame 0"""
    T = M.tables(mode)
    geo = T.geo
    cell_at = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(T.row, T.col))}
    strips = (geo.DIM_Y + M.QUEUE_ROWS - 1) // M.QUEUE_ROWS
    last_strip_row = min((strips - 1) * M.QUEUE_ROWS + 1, geo.DIM_Y - 1)
    mid = geo.DIM_Y // 2
    x0 = geo.OFFSET + np.arange(geo.DIM_X) * geo.PITCH
    straddle = int(np.flatnonzero(((x0 & 31) > 24) & (np.arange(geo.DIM_X) > geo.DIM_X // 2))[0])
    res = boundary(mode)[0].result
    strip, slot = M.queue_slots(res, mode)
    late = np.flatnonzero((strip == 3) & (slot >= 64 + 37) & (slot < 128))         # the second turn of a walk 64 slots at a time, not its first lane
    out = {"cell-0": 0, "last-cell": geo.NCELLS - 1, "last-column": cell_at[(mid, geo.DIM_X - 1)],
           "last-strip": cell_at[(last_strip_row, geo.DIM_X // 3)], "word-straddle": cell_at[(mid - 3, straddle)], "queue-second-turn": int(late[0])}
    if mode == 66:
        out["row-68"] = cell_at[(68, geo.DIM_X // 2)]
    return out


def one_closer(res):
    return (res.dc != 0) & (res.other == res.dc - 1)


def corner_only(res):
    return (res.dc != 0) & (res.corner < res.dc) & (res.side >= res.dc)


@functools.lru_cache(maxsize=None)
def one_cell(mode):
    out = []
    for k, (name, cell) in enumerate(locations(mode).items()):
        rng = np.random.default_rng([SEED, mode, 3, k])
        plan = redraw(mode, base_plan(mode), [cell], one_closer, rng, BOUNDARY_FLIPS[0], name)
        out.append(Case(mode, 3, name, plan, True, [cell]))
    return out


def seed_neighbours(mode):
    """the non-seed cell next to each seed in its row"""
    T = M.tables(mode)
    out = []
    for s in T.seeds:
        nb = s + 1 if s + 1 < T.geo.NCELLS and T.row[s + 1] == T.row[s] and T.col[s + 1] == T.col[s] + 1 and T.col[s] < T.geo.DIM_X // 2 else s - 1
        assert T.row[nb] == T.row[s] and abs(int(T.col[nb]) - int(T.col[s])) == 1 and not T.is_seed[nb]
        out.append(int(nb))
    return out


@functools.lru_cache(maxsize=None)
def seed_cases(mode):
    T = M.tables(mode)
    out = []
    for k, s in enumerate(T.seeds):
        rng = np.random.default_rng([SEED, mode, 4, k])
        plan = redraw(mode, base_plan(mode), [int(s)], corner_only, rng, BOUNDARY_FLIPS[0], f"seed-{k}")
        out.append(Case(mode, 4, f"seed-{k}", plan, True, [int(s)]))
    plan = base_plan(mode)
    restore(plan, mode, T.seeds)
    plan = repaired(mode, plan)
    nbs = seed_neighbours(mode)
    plan = redraw(mode, plan, nbs, corner_only, np.random.default_rng([SEED, mode, 4, 8]), BOUNDARY_FLIPS[0], "seed-neighbours")
    out.append(Case(mode, 4, "seed-neighbours", plan, False, nbs))
    return out


SETS = {1: boundary, 2: queue_stress, 3: one_cell, 4: seed_cases}


def cases(mode, set_no=None):
    """the cases of one set, or of sets 1 to 4 in order"""
    if set_no is not None:
        return SETS[set_no](mode)
    return [c for s in sorted(SETS) for c in SETS[s](mode)]


def split_batch(mode):
    """(unique cases, index of each of the SPLIT_FRAMES frames into them)"""
    unique = cases(mode)
    return unique, np.arange(SPLIT_FRAMES) % len(unique)


def first_difference(case, got_sym, want_sym, got_pos=None, want_pos=None):
    """None, or a message naming the mode, the case and the first differing cell with its distances from the model"""
    T = M.tables(case.mode)
    bad = got_sym != want_sym
    if got_pos is not None:
        bad = bad | (got_pos != want_pos).any(1)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    msg = f"{case}: {int(bad.sum())} cells differ, first {case.result.describe(T, i)}: symbol {got_sym[i]} for {want_sym[i]}"
    if got_pos is not None:
        msg += f", position {tuple(int(v) for v in got_pos[i])} for {tuple(int(v) for v in want_pos[i])}"
    return msg


# ------------------------------------------------------------------------------------------------ the oracle on the cases
_flood, _decode = {}, {}


def oracle_flood(case):
    """co_symbol_pass on the case's plane: (symbols, positions) by cell index"""
    key = (case.mode, case.set, case.name)
    if key not in _flood:
        n = M.tables(case.mode).geo.NCELLS
        visit = np.zeros((n, 4), np.int32)
        assert pyref.oracle_lib(case.mode).co_symbol_pass(P(case.packed), P(visit), None) == n
        order = np.argsort(visit[:, 0])
        assert (visit[order, 0] == np.arange(n)).all()
        _flood[key] = (visit[order, 3].astype(np.uint8), visit[order, 1:3].copy())
    return _flood[key]


def oracle_decode(mode, set_no):
    """oracle_decode of the set's frames in order, the colour matrix carried from frame to frame: [dict(sym, pos, chunks, mask)]"""
    key = (mode, set_no)
    if key not in _decode:
        ccm = pyref.CoCcm()
        out = []
        for c in cases(mode, set_no):
            r, chunks, mask, ccm = pyref.oracle_decode(c.frame, 0, 2, ccm, mode=mode)
            sym, col, pos = pyref.oracle_stage(mode=mode)
            out.append(dict(sym=sym, pos=pos, chunks=chunks.copy(), mask=mask))
        _decode[key] = out
    return _decode[key]
