"""The colour erasure retry (cimbar_hip_set_colour_erasure_decode -> k_colour_erasure_frame) restated in plain Python / numpy.

- `cell_means`: Cell.h:30-62 mean_rgb over the 6x6 inside each cell at the position the decoder read it (grid position + drift).
- `margins`: the classifier's confidence, colour_cases.tie_margin (second-smallest minus smallest squared distance of get_best_color) under the
  matrix in force (10 floats: 3x3 row-major + active flag; inactive = no matrix).
- `stream_bytes` / `byte_scores`: the colour stream through the geometry's interleave, four cells (2 bits each, first cell in the high bits)
  per byte; a byte's score is max over its four cells of colour_margin - margin, flagged when > 0.
- `select`: the flagged bytes ranked by score (higher first), ties to the lower position, at most max_erasures of them.
- `retry_block`: a block errors-only decoding failed is decoded again with the selected erasures (none flagged: not retried); a block it
  decoded is decoded again with none. Accepted = erasure_model.status == 1 and, with erasures, 2 * errors <= parity - e - SLACK, errors = the
  order of the Berlekamp-Massey locator.
- `retry_frame`: every colour chunk the mask lacks whose blocks are all accepted joins the mask with its bytes; the slots of colour chunks still
  missing are zero; everything else is left as it was.
"""
import numpy as np

from tests import colour_cases as C
from tests import erasure_model as E
from tests.rs_cases import syndromes

SLACK = 6          # ERASURE_SLACK (csrc/erasure.hip.inc)
SKIPPED = 0xFFFFFFFF


def default_max_erasures(geo):
    return geo.RS_PARITY - 8


def cell_means(frame, positions):
    """(N, 2) top-left (x, y) of each cell as the decoder read it -> (N, 3) uint16 sums / 36 of the 6x6 block at (x + 1, y + 1)"""
    pos = np.asarray(positions, np.int64)
    d = np.arange(6)
    ys = (pos[:, 1] + 1)[:, None, None] + d[None, :, None]
    xs = (pos[:, 0] + 1)[:, None, None] + d[None, None, :]
    win = frame[ys, xs].astype(np.int64)                                   # (N, 6, 6, 3)
    return (win.sum((1, 2)) & 0xFFFF) // 36


def matrix_of(ccm10):
    """10 floats (3x3 row-major + active flag) -> the 9-float matrix, or None where no matrix is active"""
    ccm10 = np.asarray(ccm10, np.float32).reshape(-1)
    return ccm10[:9].copy() if ccm10[9] != 0 else None


def margins(means, ccm10):
    """(N, 3) integer means -> (N,) uint32 margin under the matrix in force"""
    return C.tie_margin(np.asarray(means, np.float32), matrix_of(ccm10), C.PALETTE_B).astype(np.uint32)


def classes(means, ccm10):
    return C.best_color(np.asarray(means, np.float32), matrix_of(ccm10), C.PALETTE_B)


def stream_bytes(geo, colours):
    """(NCELLS,) colours by linear cell index -> (COL_BLOCKS, RS_BLOCK) bytes of the colour stream"""
    c = (np.asarray(colours, np.uint32)[geo.interleave_indices()] & 3).reshape(-1, 4)
    return ((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8).reshape(geo.COL_BLOCKS, geo.RS_BLOCK)


def byte_scores(geo, cell_margins, colour_margin):
    """(NCELLS,) margins -> (COL_BLOCKS, RS_BLOCK) int64 scores: max over the byte's four cells of colour_margin - margin"""
    m = np.asarray(cell_margins, np.int64)[geo.interleave_indices()].reshape(-1, 4)
    return (int(colour_margin) - m).max(1).reshape(geo.COL_BLOCKS, geo.RS_BLOCK)


def select(scores, max_erasures):
    """byte positions of the max_erasures highest scores > 0, higher score first, ties to the lower position (rank order)"""
    flagged = [k for k in range(len(scores)) if scores[k] > 0]
    flagged.sort(key=lambda k: (-int(scores[k]), k))
    return flagged[:max_erasures]


def locator_order(block, erasures, parity):
    """the order of Berlekamp-Massey's error locator over the parity - e modified syndromes (decode.c:32-118, 445-452): the errors located
    beside the erasures. 0 for a codeword."""
    block = [int(v) for v in block]
    n, e = len(block), len(erasures)
    S = [int(v) for v in syndromes(block, parity)]
    if not any(S):
        return 0
    roots = [E._div(1, E._EXP[(n - 1 - int(p)) & 0xFF]) for p in erasures]
    eloc = [1]
    if e:
        eloc = [roots[0], 1]
        for r in roots[1:]:
            eloc = [(eloc[i - 1] if i >= 1 else 0) ^ (E._mul(r, eloc[i]) if i < len(eloc) else 0) for i in range(len(eloc) + 1)]
    mod = [0] * parity
    for i, c in enumerate(eloc):
        for j in range(parity - i):
            mod[i + j] ^= E._mul(c, S[j])
    T = mod[e:]
    size = 2 * parity + 12
    loc, last = [0] * size, [0] * size
    loc[0] = last[0] = 1
    loc_order = last_order = numerrors = 0
    delay, last_disc = 1, 1
    for i in range(parity - e):
        disc = T[i]
        for j in range(1, numerrors + 1):
            disc ^= E._mul(loc[j], T[i - j])
        if not disc:
            delay += 1
            continue
        if 2 * numerrors <= i:
            for j in range(last_order, -1, -1):
                if j + delay < size:
                    last[j + delay] = E._div(E._mul(last[j], disc), last_disc)
            for j in range(delay - 1, -1, -1):
                if j < size:
                    last[j] = 0
            for j in range(min(last_order + delay + 1, size)):
                loc[j], last[j] = loc[j] ^ last[j], loc[j]
            loc_order, last_order = last_order + delay, loc_order
            numerrors = i + 1 - numerrors
            last_disc, delay = disc, 1
            continue
        for j in range(last_order, -1, -1):
            if j + delay < size:
                loc[j + delay] ^= E._div(E._mul(last[j], disc), last_disc)
        loc_order = max(loc_order, last_order + delay)
        delay += 1
    return loc_order


def errors_only_ok(block, parity):
    """the per-block flag of the decode chain: libcorrect's errors-only decode returns the message length"""
    return E.decode(block, [], parity)[0] >= 0


def retry_block(block, scores, ok, parity, max_erasures):
    """-> (status, message bytes, erasures): status 1 accepted, 0 / -1 as erasure_model.status, -2 = a failed block with nothing flagged (not retried)"""
    er = [] if ok else select(scores, max_erasures)
    if not ok and not er:
        return -2, None, er
    rc, msg, word, in_pad = E.decode(block, er, parity)
    st = E.status(rc, word, in_pad, parity)
    if st == 1 and er and 2 * locator_order(block, er, parity) > parity - len(er) - SLACK:
        st = 0
    return st, msg, er


def retry_frame(geo, colours, cell_margins, mask, chunks, colour_margin, max_erasures=None, rs_ok=None):
    """colours, cell_margins: (NCELLS,); mask, chunks ((CHUNKS, CHUNK) uint8): the frame's result without the retry -> (mask, chunks, worked).
    worked False: every colour chunk was in the mask already and nothing was looked at. rs_ok: the chain's per-block flags of the colour
    blocks ((COL_BLOCKS,), computed here when not given)."""
    e_max = default_max_erasures(geo) if max_erasures is None else int(max_erasures)
    bpc = geo.CHUNK // geo.RS_DATA
    sym_chunks = geo.SYM_BLOCKS // bpc
    col_chunks = geo.CHUNKS_PER_FRAME - sym_chunks
    mask = int(mask)
    out = np.array(chunks, np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    col_mask = ((1 << col_chunks) - 1) << sym_chunks
    if mask & col_mask == col_mask:
        return mask, out, False
    blocks = stream_bytes(geo, colours)
    scores = byte_scores(geo, cell_margins, colour_margin)
    new = mask
    for j in range(sym_chunks, geo.CHUNKS_PER_FRAME):
        if mask & (1 << j):
            continue
        good = True
        for q in range(bpc):
            cb = (j - sym_chunks) * bpc + q
            ok = errors_only_ok(blocks[cb], geo.RS_PARITY) if rs_ok is None else bool(rs_ok[cb])
            st, msg, _ = retry_block(blocks[cb], scores[cb], ok, geo.RS_PARITY, e_max)
            if st != 1:
                good = False
                break                                  # (the chunk is lost either way; the device decodes the rest, with no visible effect)
            out[j, q * geo.RS_DATA:(q + 1) * geo.RS_DATA] = msg
        if good:
            new |= 1 << j
        else:
            out[j] = 0
    return new, out, True
