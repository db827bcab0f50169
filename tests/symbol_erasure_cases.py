"""Inputs the symbol erasure tests share (tests/test_symbol_erasure_model.py on the CPU, tests/test_gpu_symbol_erasure_model.py on the GPU): a few
frames per mode, each Reed-Solomon block of which is built to put one rule of the retry to the test.

A frame is rendered from stream bytes (rs_cases.blocks_to_tiles + FrameSynth.render), so a byte can be made a "clean wrong tile": an error at
distance 0, which the retry cannot see. A cell's distance is then graded by flipping pixels inside the cell (rows and columns 1 .. 6 only: the
5x5 threshold window of a neighbouring cell never reaches them) until the oracle's threshold of the surrounding crop puts the cell's hash at
exactly the wanted distance from the tile it was rendered with, that tile still being the nearest. Nothing is guessed: `grade` searches
against co_threshold_bitplane, and tests/test_symbol_erasure_model.py checks every promise below against the model's record.

With p parity bytes, T = p // 2, E = p - 8 (the default cap) and t_sym = 6, distances 8 / 7 / 6 / 5 score 3 / 2 / 1 / 0:
  order    E wrong bytes at distance 8 behind 8 right bytes at distance 6 at lower positions: accepted only when the highest scores go first
  ties     E - 2 wrong bytes at 8, then four bytes at 7 of which the two at the lower positions are wrong: accepted only with ties to the lower
  cap      E wrong bytes at 8, one right byte at 6, one clean wrong byte: 2 * 1 <= p - E - 6 holds at exactly E erasures
  exact    E - 4 wrong bytes at 8, one wrong byte at exactly 6, one wrong byte whose nibbles are at 2 and 8, two clean wrong bytes and a right
           byte at exactly 5: 2 * 2 <= p - (E - 2) - 6 holds only when the byte at 6 is flagged, the byte at 5 is not, and the second nibble counts
  slack    E wrong bytes at 8 and two clean wrong bytes: libcorrect decodes it (status 1), 2 * 2 > p - E - 6 refuses it
  slack5   E - 1 wrong bytes at 8 and two clean wrong bytes: 4 > 3 refuses it; a slack of 5 would not
  blind    T + 1 clean wrong bytes at positions 0 .. T: fails with nothing flagged, status -2
  okblock  T clean wrong bytes and a right byte at 8: errors-only decoding accepts it, so it is decoded with no erasure
Frames: 0 clean (every chunk delivered: the retry returns at once); 1 chunk 0 = order + okblock, chunk 1 = ties, chunk 2 = cap, chunk 3 = exact
(four missing chunks: all four wavefronts retry); 2 chunk 0 = slack, chunk 1 = slack5, chunk 2 = blind + exact (all blocks but one accepted);
3 = frame 1 shifted down by one pixel (the flood pass, non-zero drift on every damaged cell); 4 symbol blocks 4 .. 7 = order, ties, cap, exact:
the kernel's four wavefronts take blocks 4r .. 4r + 3 together, so here every wavefront ranks, selects and decodes with erasures at the same
time, each block accepted only with its own score row and its own erasure list.
The group set: a pair of captures of frame 4 built the same way (clean wrong tiles that differ between the captures make disputed cells), and
discs / bands over frame 5 in the style of tests/test_gpu_capture_combine.py for groups of two and three.
"""
import functools

import numpy as np

from libcimbar_amd import framegen, geometry, modeb
from oracle import pyref
from tests import frames as F
from tests import rs_cases

MODES = [68, 67, 66]
T_SYM = 6
HEAVY, TIE, LOW, UNDER = 8, 7, 6, 5
SEED = 4100
GROUP_SEED = 1          # (its own generator: the pair does not move when a frame design is added)


class Plan:
    """stream-byte edits and gradings of one frame"""

    def __init__(self):
        self.wrong = []          # (block, byte, nibble or None, direction): a clean wrong tile; direction -1 / +1: a lower / higher symbol
        self.grades = []         # (block, byte, nibble, distance, toward): flips inside the rendered cell; toward: False any pixel, True toward the true
                                 # symbol's tile, -1 / +1 toward the tile a clean wrong edit of that direction shows
        self.marks = {}          # name -> block

    def W(self, b, k, nib=None, direction=0):
        self.wrong.append((b, k, nib, direction))

    def G(self, b, k, nib, d, toward=False):
        self.grades.append((b, k, nib, d, toward))


def _designs(geo, g):
    """name -> function(plan, block) laying the design into one block"""
    n, p = geo.RS_BLOCK, geo.RS_PARITY
    T, E = p // 2, p - 8

    def spots(count, lo=0):
        return sorted(int(v) for v in lo + g.choice(n - lo, count, replace=False))

    def order(pl, b):
        pos = spots(E + 8)
        for k in pos[:8]:
            pl.G(b, k, 0, LOW)
        for k in pos[8:]:
            pl.W(b, k); pl.G(b, k, 0, HEAVY)

    def ties(pl, b):
        pos = spots(E + 2)
        tie = pos[-4:]
        for k in pos[:-4]:
            pl.W(b, k); pl.G(b, k, 1, HEAVY)
        for i, k in enumerate(tie):
            if i < 2:
                pl.W(b, k)
            pl.G(b, k, 0, TIE)

    def cap(pl, b):
        pos = spots(E + 2)
        for k in pos[:E]:
            pl.W(b, k); pl.G(b, k, 0, HEAVY)
        pl.G(b, pos[E], 1, LOW)
        pl.W(b, pos[E + 1])

    def exact(pl, b):
        pos = spots(E + 1)
        for k in pos[:E - 4]:
            pl.W(b, k); pl.G(b, k, 0, HEAVY)
        k6, k28, c1, c2, k5 = pos[E - 4:E + 1]
        pl.W(b, k6); pl.G(b, k6, 0, LOW)
        pl.W(b, k28); pl.G(b, k28, 0, 2); pl.G(b, k28, 1, HEAVY)
        pl.W(b, c1); pl.W(b, c2)
        pl.G(b, k5, 1, UNDER)

    def slack(pl, b, e=E):
        pos = spots(e + 2)
        for k in pos[:e]:
            pl.W(b, k); pl.G(b, k, 0, HEAVY)
        pl.W(b, pos[e]); pl.W(b, pos[e + 1])

    def blind(pl, b):
        for k in range(T + 1):
            pl.W(b, k)

    def okblock(pl, b):
        pos = spots(T + 1)
        for k in pos[:T]:
            pl.W(b, k)
        pl.G(b, pos[T], 0, HEAVY)

    return dict(order=order, ties=ties, cap=cap, exact=exact, slack=slack, slack5=lambda pl, b: slack(pl, b, E - 1), blind=blind, okblock=okblock)


LAYOUT = {1: [(0, 0, "order"), (0, 1, "okblock"), (1, 1, "ties"), (2, 1, "cap"), (3, 1, "exact")],
          2: [(0, 1, "slack"), (1, 1, "slack5"), (2, 0, "blind"), (2, 1, "exact")]}      # frame -> (chunk, block in chunk, design)
ROUND = [(4, "order"), (5, "ties"), (6, "cap"), (7, "exact")]       # rendered frame 3: symbol block -> design, one round of the four wavefronts
NFRAMES = 6           # rendered: 0 .. 2 above, 3 the round, 4 and 5 for the groups


def _cell(geo, b, k, nib):
    return int(geo.interleave_indices()[(geo.RS_BLOCK * b + k) * 2 + nib])


def _crop_hash(O, crop):
    """the 8x8 hash at (4, 4) of a 16x16 crop, from the oracle's threshold of the crop (its 5x5 window stays inside)"""
    plane = np.zeros(32, np.uint8)
    O.co_threshold_bitplane(pyref.P(np.ascontiguousarray(crop)), 16, 16, 0, pyref.P(plane))
    bits = np.unpackbits(plane).reshape(16, 16)[4:12, 4:12]
    return int(np.packbits(bits.reshape(64)).view(">u8")[0])


def grade(O, geo, frame, cell, tile, d, g, toward=None):
    """in place: flip interior pixels of `cell` (rendered with `tile` = colour * 16 + symbol) until its hash is exactly d bits from the tile's and no
    other tile is as near. toward: a symbol -- only pixels where that symbol's tile differs from the rendered one are flipped."""
    tiles = [int(t) for t in np.asarray(modeb.TILE_HASHES, np.uint64)]
    masks = modeb.tile_masks()
    x, y = (int(v) for v in geo.cell_positions()[cell])
    sym, colour = tile & 15, geo.PALETTE[tile >> 4].astype(np.uint8)
    pix = [(r, c) for r in range(1, 7) for c in range(1, 7) if toward is None or masks[sym][r, c] != masks[toward][r, c]]
    pix = [pix[i] for i in g.permutation(len(pix))]
    dist = lambda: [bin(_crop_hash(O, frame[y - 4:y + 12, x - 4:x + 12]) ^ t).count("1") for t in tiles]
    now = dist()
    assert now[sym] <= min(d, 4), "a rendered cell starts at most 4 bits from its tile (border pixels, which see the neighbouring cells)"
    for r, c in pix:
        if now[sym] == d:
            break
        old = frame[y + r, x + c].copy()
        frame[y + r, x + c] = 0 if old.any() else colour
        new = dist()
        if new[sym] > d or min(v for t, v in enumerate(new) if t != sym) <= new[sym] + 2:
            frame[y + r, x + c] = old
        else:
            now = new
    assert now[sym] == d, f"cell {cell}: distance {now[sym]} reached, {d} wanted"


def _other_symbol(s, k, direction):
    """the lower (-1) / higher (+1) symbol a clean wrong tile at byte k shows instead of s: a function of the byte's place alone, so two
    captures given the same edit show the same tile"""
    assert (s >= 1) if direction < 0 else (s <= 14), "no lower / higher symbol exists"
    return (7 * s + k) % s if direction < 0 else s + 1 + (5 * k) % (15 - s)


def render(mode, plans, payload):
    """plans: one Plan (or None) per frame of the payload -> frames (n, h, w, 3), the stream bytes rendered (n, BLOCKS, RS_BLOCK)"""
    geo = geometry.for_mode(mode)
    synth = framegen.FrameSynth("cpu", mode)
    O = pyref.oracle_lib(mode)
    n = len(payload)
    true = true_blocks(geo, payload)
    blocks = true.copy()
    for f, pl in enumerate(plans):
        for b, k, nib, direction in (pl.wrong if pl else []):
            old = int(true[f, b, k])
            if direction == 0:
                new = old ^ (1 + (37 * k + 11 * b) % 255)
            else:                                      # (a function of the byte and its place alone: two captures given the same edit show the same tile)
                s = (old >> 4) & 15 if nib == 0 else old & 15
                s2 = _other_symbol(s, k, direction)
                new = (old & 0x0F) | (s2 << 4) if nib == 0 else (old & 0xF0) | s2
            blocks[f, b, k] = new
    tiles = rs_cases.blocks_to_tiles(synth, blocks.reshape(n, -1))
    true_tiles = rs_cases.blocks_to_tiles(synth, true.reshape(n, -1)).numpy()
    frames = synth.render(tiles).numpy().copy()
    tiles = tiles.numpy()
    for f, pl in enumerate(plans):
        for b, k, nib, d, toward in (pl.grades if pl else []):
            c = _cell(geo, b, k, nib)
            st = int(true_tiles[f, c]) & 15
            to = None if toward is False else st if toward is True else _other_symbol(st, k, toward)
            grade(O, geo, frames[f], c, int(tiles[f, c]), d, np.random.default_rng(SEED + c), toward=to)
    return frames, blocks


def true_blocks(geo, payload):
    n = len(payload)
    return rs_cases.encode(np.asarray(payload).reshape(n * geo.BLOCKS, geo.RS_DATA), geo.RS_PARITY).reshape(n, geo.BLOCKS, geo.RS_BLOCK)


def _group_pair_plans(geo, g, tb):
    """two captures of one frame. Block b0 of chunk 0: E bytes where capture A shows a lower wrong symbol and B the true one graded 5 bits toward
    A's (the combined cell takes A's: wrong, margin about 20; an ungraded pair would tie, and the border bits would decide), six bytes at lower
    positions where A shows a higher wrong symbol graded 7 bits toward the true one (combined: right, margin about 28), and one byte both
    captures show wrong (undisputed: an error the retry cannot see). Block b0 + 1: T + 1 bytes where B
    shows a higher wrong symbol (combined: right), so that B lacks the chunk too. Chunk 1 the same with T disputed wrong bytes and two
    undisputed wrong ones at the last two positions."""
    n, p = geo.RS_BLOCK, geo.RS_PARITY
    T, E = p // 2, p - 8
    bpc = geo.CHUNK // geo.RS_DATA
    A, B = Plan(), Plan()

    def pick(b, count, nib, direction, lo=0, hi=n):
        """byte positions lo .. hi - 1 of block b whose nibble has a lower (-1) / higher (+1) symbol to go to"""
        s = (tb[b, lo:hi] >> 4) & 15 if nib == 0 else tb[b, lo:hi] & 15
        return sorted(lo + int(v) for v in g.choice(np.flatnonzero(s >= 1 if direction < 0 else s <= 14), count, replace=False))

    for chunk, nx, ny in ((0, E, 6), (1, T, 0)):
        b = chunk * bpc
        for k in pick(b, ny, 0, +1, 0, n // 4):
            A.W(b, k, 0, +1); A.G(b, k, 0, 7, True)
        for k in pick(b, nx, 0, -1, n // 4, n - 2):
            A.W(b, k, 0, -1); B.G(b, k, 0, 5, -1)
        for k in ([n - 1] if chunk == 0 else [n - 2, n - 1]):
            nib = 0 if (int(tb[b, k]) >> 4) >= 1 else 1
            A.W(b, k, nib, -1 if (int(tb[b, k]) >> (4 if nib == 0 else 0)) & 15 else +1)
            B.wrong.append(A.wrong[-1])
        for k in pick(b + 1, T + 1, 0, +1):
            B.W(b + 1, k, 0, +1)
    return A, B


def _disc(frame, cx, cy, r, kind, seed):
    h, w, _ = frame.shape
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * min(h, w)) ** 2
    frame[d] = 255 if kind == "white" else 0 if kind == "black" else np.random.default_rng(seed).integers(0, 256, (int(d.sum()), 3), dtype=np.uint8)
    return frame


def _band(frame, x0, x1, kind, seed):
    h, w, _ = frame.shape
    ys, xs = slice(int(0.1 * h), int(0.9 * h)), slice(int(x0 * w), int(x1 * w))
    frame[ys, xs] = 255 if kind == "white" else 0 if kind == "black" else np.random.default_rng(seed).integers(0, 256, frame[ys, xs].shape, dtype=np.uint8)
    return frame


@functools.lru_cache(maxsize=None)
def case_set(mode):
    """-> dict: frames (5, h, w, 3), payload (5, FRAME_BYTES), marks (frame -> design -> symbol block), group_caps (7, h, w, 3), groups (7,),
    group_payload (3, FRAME_BYTES)"""
    geo = geometry.for_mode(mode)
    g = np.random.default_rng(SEED + mode)
    bpc = geo.CHUNK // geo.RS_DATA
    designs = _designs(geo, g)
    payload = framegen.synth_payload(NFRAMES, seed=SEED + mode, mode=mode).numpy().reshape(NFRAMES, -1)
    plans = [None] * NFRAMES
    marks = {}
    for f, lay in LAYOUT.items():
        plans[f] = Plan()
        marks[f] = {}
        for chunk, q, name in lay:
            designs[name](plans[f], chunk * bpc + q)
            marks[f][name] = chunk * bpc + q
    plans[3] = Plan()
    marks[4] = {}
    for b, name in ROUND:
        designs[name](plans[3], b)
        marks[4][name] = b
    fr, _ = render(mode, plans, payload)
    marks[3] = marks[1]
    frames = np.stack([fr[0], fr[1], fr[2], F.shift(fr[1], 1, 0), fr[3]])
    pay = np.stack([payload[0], payload[1], payload[2], payload[1], payload[3]])
    # the groups: the constructed pair, two discs, three bands
    A, B = _group_pair_plans(geo, np.random.default_rng(GROUP_SEED + mode), true_blocks(geo, payload[4:5])[0])
    pair, _ = render(mode, [A, B], np.stack([payload[4], payload[4]]))
    discs = [_disc(fr[5].copy(), cx, 0.5, 0.19, kind, 11 + c) for c, (cx, kind) in enumerate(((0.40, "noise"), (0.60, "white")))]       # (overlapping: some cells are lost in both)
    bands = [_band(fr[5].copy(), c / 3 - 0.04, (c + 1) / 3 + 0.04, kind, 21 + c) for c, kind in enumerate(("black", "noise", "white"))]
    caps = np.stack([pair[0], pair[1]] + discs + bands)
    return dict(frames=frames, payload=pay, marks=marks, group_caps=caps, groups=np.array([0, 0, 1, 1, 2, 2, 2], np.int32),
                group_payload=np.stack([payload[4], payload[5], payload[5]]))


# ---------------------------------------------------------------------------------------------- what the oracle says about the inputs
def oracle_run(mode, frames, preprocess=0, cc=2):
    """the frames through the oracle in order (the colour-correction matrix carried as a decoder carries it) -> one dict per frame: mask, chunks
    (the result without any retry), symbols, colours, positions, plane, ccm (10 floats)"""
    geo = geometry.for_mode(mode)
    O = pyref.oracle_lib(mode)
    ccm, out = None, []
    for fr in frames:
        fr = np.ascontiguousarray(fr)
        _, chunks, mask, ccm = pyref.oracle_decode(fr, preprocess, cc, ccm, mode=mode)
        sym, col, pos = pyref.oracle_stage(mode=mode)
        plane = np.zeros(geo.IMG_W * geo.IMG_H // 8, np.uint8)
        O.co_threshold_bitplane(pyref.P(fr), geo.IMG_W, geo.IMG_H, int(preprocess), pyref.P(plane))
        out.append(dict(mask=int(mask), chunks=chunks.copy(), symbols=sym, colours=col, positions=pos.astype(np.int64), plane=plane,
                        ccm=np.array(list(ccm.m) + [ccm.active], np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(mode):
    return oracle_run(mode, case_set(mode)["frames"])


@functools.lru_cache(maxsize=None)
def oracle_group_caps(mode):
    return oracle_run(mode, case_set(mode)["group_caps"])


def model_frames(mode, runs, t_sym=T_SYM, max_erasures=None, rules=None):
    """the symbol model over oracle_run's output -> [(mask, chunks, record, distances)]"""
    from tests import symbol_erasure_model as M
    geo = geometry.for_mode(mode)
    rules = M.RULES if rules is None else rules
    out = []
    for r in runs:
        d = M.cell_distances(mode, r["plane"], r["symbols"], r["positions"], True, rules, absolute=True)
        out.append(M.retry_frame(geo, r["symbols"], d, r["mask"], r["chunks"], t_sym, max_erasures, rules=rules) + (d,))
    return out


def combine_inputs(mode, runs, members):
    """combine_model.combine_cells of the captures `members` of oracle_run's output -> (cells, margins, disputed)"""
    from tests import combine_model as CM
    geo = geometry.for_mode(mode)
    grid = geo.cell_positions().astype(np.int64)
    n = len(runs)
    cells, margins = CM.combine_cells(mode, [r["plane"] for r in runs], [r["symbols"] for r in runs], [r["colours"] for r in runs],
                                      [r["positions"] - grid for r in runs], np.ones(n, np.uint8), members)
    s = np.stack([runs[c]["symbols"] & 15 for c in members])
    c = np.stack([runs[c]["colours"] for c in members])
    return cells, margins, bool((s != s[0]).any() or (c != c[0]).any())
