"""The erasure retry of the stitched decode (cimbar_hip_set_stitch_erasure -> k_stitch_erasure, k_stitch_colour_erasure) restated from the rule in
include/cimbar_hip.h ("Erasure retry in the stitched decode"), over the models that already exist:

- the decision is the stitch model's: tests/stitch_model.stitch_pair's tear record, or tests/stitch_strips_model.stitch_pair's strip records
  for strips above 1. `source` turns it into src(i), 0 = capture k, 1 = capture k + 1, per direction: direction 0 takes cell i from capture
  k + 1 where line(i) < s (s = the record's split, with strips the resolved split of the cell's strip), direction 1 the reverse.
- the confidences are the frame retries': a capture's d_sym is symbol_erasure_model.cell_distances of that capture (its own plane, drift,
  flood flag and symbols -- the stitched symbol of a cell IS its source capture's), its margin colour_erasure_model.margins of the means the
  capture's colour pass read (`capture_margins`). `by_source` picks, cell by cell, the source capture's value.
- the retries are symbol_erasure_model.retry_frame and colour_erasure_model.retry_frame on the slot's result with the setting off, the symbol
  retry first. A slot that is not live is left alone. `retry_slot` returns what the taps report as well: 0xFF / 0xFFFFFFFF rows for a retry
  that was not armed for the slot (not live, or nothing of its kind missing).

Nothing of the kernels' arithmetic is restated here.
"""
import numpy as np

from libcimbar_amd import geometry
from tests import colour_erasure_model as CE
from tests import stitch_model as SM
from tests import stitch_strips_model as SSM
from tests import symbol_erasure_model as M

DIST_SKIPPED, MARGIN_SKIPPED = 0xFF, 0xFFFFFFFF


def source(mode, axis, tear, strips_rec=None, wrong=None):
    """tear: (4,) {a, b, s, f}; strips_rec: (S, 4) for strips above 1 -> (2, NCELLS) int src per direction (0 = capture k, 1 = capture k + 1), or
    None for a pair that is no candidate. wrong="k": every cell from capture k (the mutant the case set must notice)."""
    if int(tear[0]) < 0:
        return None
    line, _, _ = SM.lines_of(mode, axis)
    if strips_rec is None:
        low = line < int(tear[2])
    else:
        rec = np.asarray(strips_rec)
        strip, _ = SSM.strips_of(mode, axis, len(rec))
        low = line < rec[strip, 2]
    src = np.stack([low, ~low]).astype(np.int64)
    return np.zeros_like(src) if wrong == "k" else src


def by_source(src, v0, v1):
    """cell by cell the source capture's value: src (NCELLS,), v0 / v1 capture k's / k + 1's (NCELLS,)"""
    return np.where(np.asarray(src) == 1, np.asarray(v1), np.asarray(v0))


def capture_margins(mode, frame, drift, flooded, ccm10):
    """the colour margins of one capture as its colour pass saw the cells: the 6x6 mean at the drifted position where the capture took a flood
    pass, at the grid position otherwise, under the capture's matrix in force (10 floats)"""
    grid = geometry.for_mode(mode).cell_positions().astype(np.int64)
    return CE.margins(CE.cell_means(frame, grid + (np.asarray(drift, np.int64).reshape(-1, 2) if flooded else 0)), ccm10)


def retry_slot(mode, src, cells, dist, marg, mask, chunks, live=True, t_sym=0, colour_margin=0, sym_max=None, col_max=None, rules=M.RULES):
    """One slot. src: (NCELLS,) 0 / 1 (None: not live); cells: (NCELLS,) the stitched cells colour << 4 | symbol (TAP_STITCH_CELLS or the stitch
    model's); dist, marg: pairs (capture k's, capture k + 1's) of (NCELLS,) arrays; mask, chunks: the slot with the setting off; t_sym /
    colour_margin <= 0: that retry is not armed -> (mask, chunks, distances (NCELLS,) uint8, margins (NCELLS,) uint32)"""
    geo = geometry.for_mode(mode)
    mask = int(mask)
    out = np.array(chunks, np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    tap_d = np.full(geo.NCELLS, DIST_SKIPPED, np.uint8)
    tap_m = np.full(geo.NCELLS, MARGIN_SKIPPED, np.uint32)
    if not live or src is None:
        return mask, out, tap_d, tap_m
    cells = np.asarray(cells, np.uint8)
    if t_sym > 0:
        d = by_source(src, dist[0], dist[1])
        mask, out, rec = M.retry_frame(geo, cells & 15, d, mask, out, t_sym, sym_max, rules=rules)
        if rec is not None:
            tap_d = d.astype(np.uint8)
    if colour_margin > 0:
        m = by_source(src, marg[0], marg[1])
        mask, out, worked = CE.retry_frame(geo, cells >> 4, m, mask, out, colour_margin, None if col_max is None or col_max < 0 else col_max)
        if worked:
            tap_m = m.astype(np.uint32)
    return mask, out, tap_d, tap_m


def retry_batch(mode, axis, tears, cells, dists, margs, smasks, schunks, strips_recs=None, wrong=None, **kw):
    """every slot of a batch of n captures. tears (n - 1, 4); cells (2 (n - 1), NCELLS); dists, margs: per capture (n, NCELLS) (margs may be
    None when the colour retry is not armed); smasks, schunks: the setting-off result -> (smasks, schunks, distances, margins) over the slots"""
    geo = geometry.for_mode(mode)
    slots = 2 * len(tears)
    om, oc = np.zeros(slots, np.uint32), np.zeros((slots, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    od, og = np.zeros((slots, geo.NCELLS), np.uint8), np.zeros((slots, geo.NCELLS), np.uint32)
    for k in range(len(tears)):
        src = source(mode, axis, tears[k], None if strips_recs is None else strips_recs[k], wrong)
        for d in range(2):
            g = 2 * k + d
            mg = (None, None) if margs is None else (margs[k], margs[k + 1])
            om[g], oc[g], od[g], og[g] = retry_slot(mode, None if src is None else src[d], cells[g], (dists[k], dists[k + 1]), mg, smasks[g],
                                                    schunks[g], src is not None, **kw)
    return om, oc, od, og
