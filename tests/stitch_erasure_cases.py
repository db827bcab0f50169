"""Inputs the stitched-erasure tests share (tests/test_stitch_erasure_model.py on the CPU, tests/test_gpu_stitch_erasure.py on the GPU).

Frame B is frame 1 of tests/symbol_erasure_cases.case_set: rendered by its `render` / `grade` with the designs "order" + "okblock", "ties",
"cap" and "exact" in symbol chunks 0 .. 3, so errors-only decoding loses those four chunks and the symbol retry wins them back only by the
rules. A block's cells are spread over half the frame (the interleave has two partitions, the upper and the lower half of the cells): on axis 1
every failing block has graded cells on both sides of any split, so the retry must read both captures; on axis 0 with the "across" tears the
split lies near the partition boundary and some failing block's graded cells all lie on one side.

The colour part: in one colour block of B (and of C), E = parity - 8 bytes -- more than errors-only decoding corrects, exactly what the default
cap erases -- have their four cells repainted with a mix of their colour and another palette colour, a little more than half way to
the other one, pulled half way to grey: of the other colours and a few mixes, the one that leaves the smallest margin on the wrong side. (Grey alone does not lower the margin: the classifier works on relative colours and stretches any tint
back to full saturation. What lowers it is nearness to the boundary between two colours.) The classifier picks the wrong colour with a
margin below COLOUR_MARGIN_SUGGESTED, so errors-only decoding loses the block's chunk and the colour retry finds the bytes. Cells the symbol designs touched, and their neighbours, are left alone (their graded distances depend on the pixels around them).

Frames A, D and E are clean; C is clean but for its colour block (Cd). Batches of four captures, torn with stitch_cases.torn_pair at the
"across" and "midcell" tears on both axes in both directions. Three pairs cannot hold four kinds of pair, so there are two lay-outs:
  "across":  [A, T1, T2, Cd], T1 / T2 = torn_pair(A, B, Cd): pair 0 stitches to A (a live slot that is complete), pair 1 to B (slot 2 +
             direction: needs the symbol retry and the colour retry), pair 2 to Cd (slot 4 + direction: needs the colour retry only)
  "midcell": [D, E, T1, T2], T1 / T2 = torn_pair(A, B, C): pairs 0 and 1 are no candidates, pair 2 stitches to B in slot 4 + direction
tests/test_stitch_erasure_model.py checks these promises against the oracle.
"""
import functools

import numpy as np

from libcimbar_amd import framegen, geometry
from tests import colour_erasure_cases as CEC
from tests import colour_erasure_model as CE
from tests import stitch_cases as SC
from tests import symbol_erasure_cases as K

MODES = K.MODES
T_SYM = K.T_SYM
MARGIN = CEC.MARGIN
SEED = 5200
GREY, PULL, MIXES = 128.0, 0.5, (0.52, 0.54, 0.57, 0.6)  # a repainted cell: grey + PULL * ((1 - mix) * its colour + mix * another palette colour - grey)
CASES = [(name, axis, direction) for name in ("across", "midcell") for axis in (0, 1) for direction in (0, 1)]
TARGET = ("across", 1, 0)           # the case the sensitivity checks run on: axis 1, both captures hold graded cells of every failing block


def case_id(case):
    return "%s-axis%d-dir%d" % case


def _touched(geo, frame, clean):
    """the cells whose 8x8 pixels differ from the clean rendering, and the cells next to them"""
    xy = geo.cell_positions()
    at = {(int(x), int(y)): i for i, (x, y) in enumerate(xy)}
    out = set()
    for i, (x, y) in enumerate(xy):
        if (frame[y:y + 8, x:x + 8] != clean[y:y + 8, x:x + 8]).any():
            for dx in (-geo.PITCH, 0, geo.PITCH):
                for dy in (-geo.PITCH, 0, geo.PITCH):
                    out.add(at.get((int(x) + dx, int(y) + dy), i))
    return out


def desaturate(mode, frame, block, seed, avoid=()):
    """in place: E bytes of colour block `block` repainted as described above -> the byte positions"""
    geo = geometry.for_mode(mode)
    g = np.random.default_rng(seed)
    il = geo.interleave_indices()
    xy = geo.cell_positions()
    cells_of = lambda k: [int(il[(geo.RS_BLOCK * block + k) * 4 + q]) for q in range(4)]
    free = [k for k in range(geo.RS_BLOCK) if not any(c in avoid for c in cells_of(k))]
    pos = sorted(int(free[i]) for i in g.choice(len(free), geo.RS_PARITY - 8, replace=False))
    pal = np.asarray(geo.PALETTE, np.float64)
    none = np.zeros(10, np.float32)
    for k in pos:
        for c in cells_of(k):
            x, y = (int(v) for v in xy[c])
            cell = frame[y:y + 8, x:x + 8]
            ink = cell.any(axis=2)
            have = int(np.argmin(((pal - cell[ink][0].astype(np.float64)) ** 2).sum(1)))
            # the partner and the mix that leave the smallest margin on the wrong side of a boundary, judged without a matrix (the captures'
            # own matrices move it a little: the CPU test checks what the oracle makes of it)
            best = None
            for other in range(len(pal)):
                for mix in MIXES:
                    if other == have:
                        continue
                    cell[ink] = np.rint(GREY + PULL * ((1 - mix) * pal[have] + mix * pal[other] - GREY)).astype(np.uint8)
                    mean = CE.cell_means(frame, np.array([[x, y]]))
                    key = (int(CE.classes(mean, none)[0]) == have, int(CE.margins(mean, none)[0]))
                    if best is None or key < best[0]:
                        best = (key, cell[ink][0].copy())
            cell[ink] = best[1]
    return pos


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    """-> dict: frames A, B, C (clean), Cd, D, E; pay: name -> (FRAME_BYTES,) payload (Cd's is C's); colour_block, and the repainted byte
    positions of B and Cd"""
    import torch
    geo = geometry.for_mode(mode)
    ks = K.case_set(mode)
    synth = framegen.FrameSynth("cpu", mode)
    # A, B, C are consecutive frames of one stream, as a display shows them: a torn capture predicts the header cells of its lower frame from
    # the header of its upper one (the colour-correction matrix is fitted to that prediction), which holds only for consecutive block ids
    A, B = ks["frames"][0].copy(), ks["frames"][1].copy()
    clean = synth.frames_from_payload(torch.from_numpy(np.ascontiguousarray(ks["payload"][1:3]))).numpy().copy()
    clean_b, C = clean[0], clean[1]
    other = framegen.synth_payload(2, seed=SEED + mode, mode=mode)
    Dd, E = synth.frames_from_payload(other).numpy().copy()
    pay = np.stack([ks["payload"][0], ks["payload"][2]] + list(other.numpy().reshape(2, -1)))
    cb = geo.COL_BLOCKS // 2 + 1          # (the second block of a colour chunk in the lower partition)
    pos_b = desaturate(mode, B, cb, SEED + 1, _touched(geo, B, clean_b))
    Cd = C.copy()
    pos_c = desaturate(mode, Cd, cb, SEED + 2)
    return dict(A=A, B=B, C=C, Cd=Cd, D=Dd, E=E, pay=dict(A=pay[0], B=ks["payload"][1], C=pay[1], Cd=pay[1], D=pay[2], E=pay[3]),
                colour_block=cb, pos_b=pos_b, pos_c=pos_c)


def batch(mode, case):
    """-> (captures (4, h, w, 3), names of the frames shown, dict: b = the slot of B, cd = the slot of Cd or None, dead = the slots of pairs that
    are no candidates, complete = a live slot that lacks nothing, or None)"""
    name, axis, direction = case
    f = frames_of(mode)
    p1, p2 = SC.tear_pixels(mode, axis, name)
    if name == "across":
        t1, t2 = SC.torn_pair(f["A"], f["B"], f["Cd"], axis, p1, p2, direction)
        return np.stack([f["A"], t1, t2, f["Cd"]]), ("A", "B", "Cd"), dict(b=2 + direction, cd=4 + direction, dead=(), complete=0 + direction)
    t1, t2 = SC.torn_pair(f["A"], f["B"], f["C"], axis, p1, p2, direction)
    return np.stack([f["D"], f["E"], t1, t2]), ("A", "B", "C", "D", "E"), dict(b=4 + direction, cd=None, dead=(0, 1, 2, 3), complete=None)


def genuine(mode, shown, smasks, schunks):
    """None if every chunk in every mask is that chunk of one of the frames shown and every other slot of a chunk is zero, else a message"""
    geo = geometry.for_mode(mode)
    pay = frames_of(mode)["pay"]
    sc = np.asarray(schunks).reshape(len(smasks), geo.CHUNKS_PER_FRAME, geo.CHUNK)
    for g in range(len(smasks)):
        for j in range(geo.CHUNKS_PER_FRAME):
            if (int(smasks[g]) >> j) & 1:
                if not any((sc[g, j] == pay[nm].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[j]).all() for nm in shown):
                    return f"slot {g} chunk {j}: in the mask, and no shown frame's chunk"
            elif sc[g, j].any():
                return f"slot {g} chunk {j}: not in the mask, not zero"
    return None
