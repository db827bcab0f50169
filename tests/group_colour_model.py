"""The colour vote of the group decode and the group colour retry (cimbar_hip_set_group_colour_vote -> k_group_colour, k_group_colour_retry)
restated in plain Python / numpy from the rule in include/cimbar_hip.h, not from the kernels.

For one group with members c = 0 .. m - 1 and one cell:
- col_c: the class k_colors gave the member's cell; marg_c: its classifier margin (colour_erasure_model.margins: what TAP_COLOUR_MARGIN defines)
- w_c = marg_c + 1; score(k) = the sum of w_c over the members with col_c == k
- a cell whose members all agree on the colour is settled as before: no margin (NONE), no weight
- a disputed cell takes the colour with the largest score, ties to the lowest colour index; gm = the largest score minus the second-largest,
  a colour nobody voted for scoring 0 (`vote`)
The symbol side of the combined cells does not depend on any of this.

The group decode over the voted cells (`decode_group`): the combined cells' errors-only Reed-Solomon decode and aligned_stream's bookkeeping over the
symbol blocks, then the colour blocks, with one state (`combined_mask`: a chunk is delivered when all its blocks decoded and the last block of
the chunk before it did); chunk j of the group = the combined decode's where it delivered it, else the lowest-index member's that delivered
it. The group colour retry (`retry_colour`), armed by the colour erasure setting: for the colour chunks the group mask still lacks, a colour-stream
byte's score is max over its four cells of colour_margin - gm, a cell without a dispute contributing nothing; flagged when > 0; the max_erasures
highest scores become erasures, ties to the lower byte; retry and acceptance are colour_erasure_model.retry_block's; chunks already in the mask are
never rewritten and the slots of chunks still missing are zero. A group whose members agree on every cell (symbol and colour) is skipped by the
group decode altogether: the members' chunks are the answer.
"""
import numpy as np

from tests import colour_erasure_model as CE
from tests import erasure_model as E
from tests import symbol_erasure_model as SM

NONE = 0xFFFFFFFF
NCOLOURS = 4


def vote(colours, margins):
    """colours, margins: (m, NCELLS) of the members in member order -> (colour (NCELLS,) uint8, gm (NCELLS,) uint32, weights (m, NCELLS) uint32)"""
    col = np.asarray(colours, np.int64)
    w = np.asarray(margins, np.int64) + 1
    disputed = (col != col[0]).any(axis=0)
    score = np.stack([(w * (col == k)).sum(axis=0) for k in range(NCOLOURS)])          # (NCOLOURS, NCELLS)
    assert int(score.max(initial=0)) < 1 << 32
    win = score.argmax(axis=0)                                                         # (the first maximum: ties to the lowest colour index)
    ranked = np.sort(score, axis=0)
    gm = ranked[-1] - ranked[-2]
    return (np.where(disputed, win, col[0]).astype(np.uint8), np.where(disputed, gm, NONE).astype(np.uint32),
            np.where(disputed[None, :], w, 0).astype(np.uint32))


def plurality_colour(colours, distances=None):
    """the rule the vote replaces (combine_model.combine_cells' colour half): the plurality of col_c; a tie goes to the colour of the tied member
    with the smallest distance (m, NCELLS) to the chosen symbol (None: all equal), then to the lowest member -> (NCELLS,) uint8"""
    col = np.asarray(colours, np.int64)
    m, n = col.shape
    d = np.zeros((m, n), np.int64) if distances is None else np.asarray(distances, np.int64)
    votes = np.stack([(col == col[c]).sum(axis=0) for c in range(m)])                  # votes[c] = members sharing member c's colour
    tied = votes == votes.max(axis=0)
    key = np.where(tied, d * m + np.arange(m)[:, None], np.iinfo(np.int64).max)
    return col[key.argmin(axis=0), np.arange(n)].astype(np.uint8)


def _ok_flags(blocks, parity, rs_ok):
    return [SM.errors_only_ok(blocks[b], parity) if rs_ok is None else bool(rs_ok[b]) for b in range(len(blocks))]


def combined_mask(geo, sym_blocks, col_blocks, rs_ok=None):
    """aligned_stream over the errors-only flags of the symbol blocks, then the colour blocks, one state -> (mask, flags of all blocks)"""
    bpc = geo.CHUNK // geo.RS_DATA
    ok = _ok_flags(list(sym_blocks) + list(col_blocks), geo.RS_PARITY, rs_ok)
    mask, carried = 0, False
    for j in range(geo.CHUNKS_PER_FRAME):
        mine = ok[j * bpc:(j + 1) * bpc]
        if all(mine) and not carried:
            mask |= 1 << j
        carried = not mine[-1]
    return mask, ok


def byte_scores(geo, gm, colour_margin):
    """(NCELLS,) group colour margins -> (COL_BLOCKS, RS_BLOCK) int64 scores; a byte none of whose cells is disputed scores far below 0"""
    g = np.asarray(gm, np.int64)[geo.interleave_indices()].reshape(-1, 4)
    sc = np.where(g == NONE, np.iinfo(np.int32).min, int(colour_margin) - g)
    return sc.max(axis=1).reshape(geo.COL_BLOCKS, geo.RS_BLOCK)


def retry_colour(geo, colour, gm, gmask, gchunks, ok, colour_margin, max_erasures=None):
    """the group colour retry over the voted cells. gmask / gchunks ((CHUNKS, CHUNK)): the group's result after the fill; ok: the combined
    decode's flags of all blocks -> (gmask, gchunks)"""
    e_max = CE.default_max_erasures(geo) if max_erasures is None or max_erasures < 0 else int(max_erasures)
    bpc = geo.CHUNK // geo.RS_DATA
    sym_chunks = geo.SYM_BLOCKS // bpc
    out = np.array(gchunks, np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    blocks = CE.stream_bytes(geo, colour)
    scores = byte_scores(geo, gm, colour_margin)
    new = int(gmask)
    for j in range(sym_chunks, geo.CHUNKS_PER_FRAME):
        if (int(gmask) >> j) & 1:
            continue
        good = True
        for q in range(bpc):
            cb = (j - sym_chunks) * bpc + q
            st, msg, _ = CE.retry_block(blocks[cb], scores[cb], ok[geo.SYM_BLOCKS + cb], geo.RS_PARITY, e_max)
            if st != 1:
                good = False
                break
            out[j, q * geo.RS_DATA:(q + 1) * geo.RS_DATA] = msg
        if good:
            new |= 1 << j
        else:
            out[j] = 0
    return new, out


def decode_group(geo, symbols, colour, gm, member_masks, member_chunks, disputed=True, colour_margin=0, max_erasures=None, rs_ok=None):
    """symbols: (NCELLS,) the combined cells' symbols; colour, gm: the group's colours and colour margins (`vote`, or a plurality colour with
    gm None); member_masks / member_chunks: the members' per-capture results in member order; disputed: whether any cell of the group differs
    between members in symbol or colour; colour_margin > 0 arms the group colour retry (only with gm given)
    -> (gmask, gchunks (CHUNKS, CHUNK) uint8, the combined decode's own mask)"""
    out = np.zeros((geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    mmask = 0
    for mk in member_masks:
        mmask |= int(mk)
    cmask, ok = 0, None
    if disputed:
        sym_blocks = SM.stream_bytes(geo, symbols)
        col_blocks = CE.stream_bytes(geo, colour)
        cmask, ok = combined_mask(geo, sym_blocks, col_blocks, rs_ok)
        bpc = geo.CHUNK // geo.RS_DATA
        allb = list(sym_blocks) + list(col_blocks)
        for j in range(geo.CHUNKS_PER_FRAME):
            if (cmask >> j) & 1:
                for q in range(bpc):
                    out[j, q * geo.RS_DATA:(q + 1) * geo.RS_DATA] = E.decode(allb[j * bpc + q], [], geo.RS_PARITY)[1]
    for j in range(geo.CHUNKS_PER_FRAME):
        if not (cmask >> j) & 1 and (mmask >> j) & 1:
            c = next(c for c in range(len(member_masks)) if (int(member_masks[c]) >> j) & 1)
            out[j] = np.asarray(member_chunks[c], np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[j]
    gmask = (cmask | mmask) & geo.FULL_MASK
    if disputed and gm is not None and colour_margin > 0:
        gmask, out = retry_colour(geo, colour, gm, gmask, out, ok, colour_margin, max_erasures)
    return gmask, out, cmask
