"""The symbol erasure retry (cimbar_hip_set_erasure_decode -> k_erasure_frame, and the group decode's retry, group_end_body with e_on) restated in
plain Python / numpy from the two texts that specify it: the header comment of k_erasure_frame (csrc/erasure.hip.inc) and the
cimbar_hip_set_erasure_decode / "group decode" paragraphs of include/cimbar_hip.h.

The frame retry, for a frame whose symbol chunks are not all in the mask:
- confidence: d_sym(c) = popcount(8x8 hash of the bit plane at the cell's final position ^ tile hash of the cell's decoded symbol); the final
  position is the grid position plus the drift where the frame went through the flood pass, the grid position otherwise (`cell_distances`,
  over combine_model.cell_hashes and modeb.TILE_HASHES).
- score: a symbol-stream byte comes from two cells (high nibble first, geometry.interleave_indices order); its score is max over them of
  d_sym - t_sym + 1, flagged when > 0 (`byte_scores`, `stream_bytes`).
- selection: the max_erasures highest scores, ties to the lower byte position (colour_erasure_model.select: shared with the colour retry).
- retry: a block errors-only decoding failed is decoded with those erasures (none flagged: not retried, status -2); a block it decoded is
  decoded again with none. Accepted = erasure_model.status == 1 and, with erasures, 2 * errors <= parity - e - SLACK.
- chunk: a chunk the mask lacks whose blocks are all accepted joins the mask with its bytes; the slots of chunks still missing are zero;
  everything else is untouched (`retry_frame`).
The group retry (`retry_group`): the symbol chunks neither the combined decode nor a member delivered are retried on the combined cells; only
bytes with a symbol-disputed cell (margin != 0xFFFF) are flagged, smallest margin first (a byte's margin = the smaller of its two cells'), then
stream position, at most max_erasures; acceptance as above; group chunk j = the combined decode's where it delivered it, else the lowest-index
member's that delivered it, else the retry's.

What the two texts leave open, resolved from the kernels:
- the hash window is the 8x8 block whose top-left pixel is the cell's position (the kernel reads a 10x10 window one pixel up and left and hashes
  its centre); the symbol's low four bits index the tile.
- "errors" in the slack rule = the order of Berlekamp-Massey's locator (colour_erasure_model.locator_order), known before the Chien search.
- the retry decodes every block of a missing chunk, also after one has failed; nothing of that is visible in the outputs.
- the group retry runs only for groups with a disputed cell (any cell whose members disagree on symbol or colour); without one, no byte could
  be flagged anyway. The combined decode's own mask follows aligned_stream's rule: a chunk is delivered when all its blocks decoded and the
  LAST block of the chunk before it did (`combined_symbol_mask`).
- on a frame that did not take the flood pass the drift the flood would produce is zero by the fast path's condition (DESIGN.md "fast path"), so
  "grid position" and "final position" name the same pixel there: the `position` switch below can only show on flooded frames.

Every rule is a switch (`rules=`; RULES holds the specified behaviour, MUTANTS / GROUP_MUTANTS one deviation each) so that the case set's
sensitivity can be shown on the CPU (tests/test_symbol_erasure_model.py). Reed-Solomon results are cached per (block, erasures): the mutants
re-decode few new blocks.
"""
import numpy as np

from libcimbar_amd import geometry, modeb
from tests import colour_erasure_model as CE
from tests import combine_model as CM
from tests import erasure_model as E

MARGIN_NONE = CM.MARGIN_NONE

RULES = dict(
    position="final",      # "swapped": the grid position on flooded frames, the drifted one on the others
    window=(0, 0),         # (dx, dy) added to the hash window's origin
    pairing=0,             # 1: byte k is scored from stream cells 2k + 1, 2k + 2
    bias=0,                # score = d - t_sym + 1 + bias
    nibble="max",          # "first": the first nibble's cell alone
    order="highest",       # "lowest": lowest score first
    ties="lower",          # "higher": ties to the higher byte position
    cap=0,                 # erasures per block = max_erasures + cap
    rows="own",            # blocks 4r .. 4r + 3 are decoded together, one per wavefront. "shared": a wavefront ranks with the score row of
                           # wavefront 0's block of its round, "shared_prev": with the row of the wavefront before it -- where that block is
                           # itself a failed block of a missing chunk, i.e. one that is being retried with erasures at the same time
    unflagged="skip",      # "retry": a failed block with nothing flagged takes the max_erasures best-ranked bytes anyway (retrying it with no
                           #          erasure is errors-only again and changes no output)
    ok_blocks="none",      # "erasures": a block errors-only decoding accepted is decoded with the selected erasures too
    slack=CE.SLACK,        # None: no slack rule; 5 / 7: off by one
    chunk="all",           # "but_one": a chunk with one block still failing is delivered
    rezero=True,           # False: the slot of a chunk still missing keeps the blocks written into it
    # the group retry
    g_order="margin",      # "position": stream position alone; "largest": largest margin first
    g_undisputed=False,    # True: undisputed cells' bytes are flagged too
    g_cap=0,
)
MUTANTS = [("position", "swapped"), ("window", (1, 0)), ("window", (0, 1)), ("pairing", 1), ("bias", 1), ("bias", -1), ("nibble", "first"),
           ("order", "lowest"), ("ties", "higher"), ("cap", 1), ("cap", -1), ("rows", "shared"), ("rows", "shared_prev"), ("unflagged", "retry"), ("ok_blocks", "erasures"),
           ("slack", None), ("slack", 5), ("slack", 7), ("chunk", "but_one"), ("rezero", False)]
GROUP_MUTANTS = [("g_order", "position"), ("g_order", "largest"), ("g_undisputed", True), ("g_cap", 1), ("g_cap", -1)]


def rules_with(**kw):
    assert set(kw) <= set(RULES), kw
    return dict(RULES, **kw)


def _popcount64(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def cell_distances(mode, bitplane, symbols, positions_or_drift, flooded, rules=RULES, absolute=False):
    """-> (NCELLS,) int64 d_sym. bitplane: the frame's TAP_BITPLANE bytes / co_threshold_bitplane's output. positions_or_drift: (NCELLS, 2) drift
    (TAP_DRIFT), or with absolute=True the cells' top-left positions (the oracle's co_last_positions)."""
    geo = geometry.for_mode(mode)
    drift = np.asarray(positions_or_drift, np.int64).reshape(-1, 2)
    if absolute:
        drift = drift - geo.cell_positions().astype(np.int64)
    use = bool(flooded) if rules["position"] == "final" else not bool(flooded)
    eff = (drift if use else np.zeros_like(drift)) + np.asarray(rules["window"], np.int64)[None, :]
    h = CM.cell_hashes(mode, bitplane, eff, True)
    tiles = np.asarray(modeb.TILE_HASHES, np.uint64)
    return _popcount64(h ^ tiles[np.asarray(symbols, np.int64) & 15])


def _stream_pairs(geo, per_cell, rules=RULES):
    s = np.asarray(per_cell)[geo.interleave_indices()]
    if rules["pairing"]:
        s = np.roll(s, -int(rules["pairing"]))
    return s.reshape(-1, 2)


def stream_bytes(geo, symbols):
    """(NCELLS,) symbols by linear cell index -> (SYM_BLOCKS, RS_BLOCK) bytes of the symbol stream"""
    s = (np.asarray(symbols, np.uint32)[geo.interleave_indices()] & 15).reshape(-1, 2)
    return ((s[:, 0] << 4) | s[:, 1]).astype(np.uint8).reshape(geo.SYM_BLOCKS, geo.RS_BLOCK)


def byte_scores(geo, distances, t_sym, rules=RULES):
    """(NCELLS,) distances -> (SYM_BLOCKS, RS_BLOCK) int64 scores: max over the byte's two cells of d - t_sym + 1"""
    d = _stream_pairs(geo, np.asarray(distances, np.int64), rules) - int(t_sym) + 1 + int(rules["bias"])
    return (d[:, 0] if rules["nibble"] == "first" else d.max(1)).reshape(geo.SYM_BLOCKS, geo.RS_BLOCK)


def _select(scores, e_max, rules, force=False):
    """rank order; the specified rule is colour_erasure_model.select"""
    if rules["order"] == "highest" and rules["ties"] == "lower" and not force:
        return CE.select(scores, e_max)
    sgn = -1 if rules["order"] == "highest" else 1
    tie = 1 if rules["ties"] == "lower" else -1
    flagged = [k for k in range(len(scores)) if force or scores[k] > 0]
    flagged.sort(key=lambda k: (sgn * int(scores[k]), tie * k))
    return flagged[:max(e_max, 0)]


_rs_cache = {}


def rs_decode(block, erasures, parity):
    """-> (status -1 / 0 / 1 of erasure_model.status, message bytes, errors beside the erasures); cached"""
    key = (np.asarray(block, np.uint8).tobytes(), tuple(int(k) for k in erasures), int(parity))
    if key not in _rs_cache:
        rc, msg, word, in_pad = E.decode(block, list(key[1]), parity)
        st = E.status(rc, word, in_pad, parity)
        nerr = CE.locator_order(block, list(key[1]), parity) if st == 1 and key[1] else 0
        _rs_cache[key] = (st, msg, nerr)
    return _rs_cache[key]


def errors_only_ok(block, parity):
    key = (np.asarray(block, np.uint8).tobytes(), "ok", int(parity))
    if key not in _rs_cache:
        _rs_cache[key] = CE.errors_only_ok(block, parity)
    return _rs_cache[key]


def _accept(st, e, nerr, parity, rules):
    if st == 1 and e > 0 and rules["slack"] is not None and 2 * nerr > parity - e - rules["slack"]:
        return 0
    return st


def _retry_block(block, erasures, ok, parity, rules):
    """-> (status, message): -2 = a failed block with no erasure"""
    if not ok and not erasures:
        return -2, None
    st, msg, nerr = rs_decode(block, erasures, parity)
    return _accept(st, len(erasures), nerr, parity, rules), msg


def _chunks_from_blocks(geo, mask, out, missing, status, msgs, chunk_rule, rezero):
    """the chunk rule over the symbol chunks in `missing` (bit set): -> the bits gained; `out` is filled / zeroed in place"""
    bpc = geo.CHUNK // geo.RS_DATA
    gained = 0
    for j in range(geo.SYM_BLOCKS // bpc):
        if not (missing >> j) & 1:
            continue
        bad = 0
        for q in range(bpc):
            b = j * bpc + q
            if status[b] == 1:
                out[j, q * geo.RS_DATA:(q + 1) * geo.RS_DATA] = msgs[b]
            else:
                bad += 1
        if bad == 0 or (chunk_rule == "but_one" and bad == 1):
            gained |= 1 << j
        elif rezero:
            out[j] = 0
    return gained


def retry_frame(geo, symbols, distances, mask, chunks, t_sym, max_erasures=None, rs_ok=None, rules=RULES):
    """symbols, distances: (NCELLS,); mask, chunks ((CHUNKS_PER_FRAME, CHUNK) uint8): the frame's result without the retry; rs_ok: the chain's
    flags of the symbol blocks ((SYM_BLOCKS,), worked out with errors_only_ok when None) -> (mask, chunks, record). record: None when every
    symbol chunk was in the mask (the retry returns at once), else one dict per symbol block: status (2 = its chunk was delivered already,
    -2 = failed with nothing flagged, else -1 / 0 / 1), erasures (rank order), ok, scores."""
    e_max = CE.default_max_erasures(geo) if max_erasures is None or max_erasures < 0 else int(max_erasures)
    bpc = geo.CHUNK // geo.RS_DATA
    sym_chunks = geo.SYM_BLOCKS // bpc
    sym_mask = (1 << sym_chunks) - 1
    mask = int(mask)
    out = np.array(chunks, np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    if mask & sym_mask == sym_mask:
        return mask, out, None
    p = geo.RS_PARITY
    blocks = stream_bytes(geo, symbols)
    scores = byte_scores(geo, distances, t_sym, rules)
    missing = sym_mask & ~mask
    status, msgs, record = {}, {}, []
    walked = [bool((missing >> (b // bpc)) & 1) for b in range(geo.SYM_BLOCKS)]
    oks = [None if not walked[b] else errors_only_ok(blocks[b], p) if rs_ok is None else bool(rs_ok[b]) for b in range(geo.SYM_BLOCKS)]
    for b in range(geo.SYM_BLOCKS):
        if not walked[b]:
            record.append(dict(status=2, erasures=[], ok=None, scores=None))
            continue
        ok = oks[b]
        row = scores[b]
        other = b - b % 4 if rules["rows"] == "shared" else b - 1 if rules["rows"] == "shared_prev" else b
        if b % 4 and other != b and walked[other] and not oks[other]:
            row = scores[other]
        er = []
        if not ok or rules["ok_blocks"] == "erasures":
            er = _select(row, e_max + rules["cap"], rules)
            if not ok and not er and rules["unflagged"] == "retry":
                er = _select(row, e_max + rules["cap"], rules, force=True)
        st, msg = _retry_block(blocks[b], er, ok, p, rules)
        status[b], msgs[b] = st, msg
        record.append(dict(status=st, erasures=er, ok=ok, scores=scores[b]))
    gained = _chunks_from_blocks(geo, mask, out, missing, status, msgs, rules["chunk"], rules["rezero"])
    return mask | gained, out, record


def combined_symbol_mask(geo, blocks, rs_ok=None):
    """the symbol bits of the combined decode's own mask: aligned_stream over the errors-only flags of the symbol blocks -- a chunk is delivered
    when all its blocks decoded and the last block of the chunk before it did (a bad last block leaves the bad mark for the next chunk)"""
    bpc = geo.CHUNK // geo.RS_DATA
    ok = [errors_only_ok(blocks[b], geo.RS_PARITY) if rs_ok is None else bool(rs_ok[b]) for b in range(geo.SYM_BLOCKS)]
    m, carried = 0, False
    for j in range(geo.SYM_BLOCKS // bpc):
        mine = ok[j * bpc:(j + 1) * bpc]
        if all(mine) and not carried:
            m |= 1 << j
        carried = not mine[-1]
    return m, ok


def _group_select(keys, e_max, rules):
    flag = [k for k in range(len(keys)) if rules["g_undisputed"] or keys[k] != MARGIN_NONE]
    if rules["g_order"] == "margin":
        flag.sort(key=lambda k: (int(keys[k]), k))
    elif rules["g_order"] == "largest":
        flag.sort(key=lambda k: (-int(keys[k]), k))
    return flag[:max(e_max + rules["g_cap"], 0)]


def retry_group(geo, cells, margins, gmask, gchunks, member_masks, member_chunks, max_erasures=None, rs_ok=None, disputed=True, rules=RULES):
    """cells, margins: combine_model.combine_cells of the group; gmask, gchunks: the group's result with the retry off; member_masks /
    member_chunks: the members' results with the retry on, in member order; disputed: whether any cell of the group is disputed in symbol or
    colour (False: the group decode is skipped and the members' chunks are the answer) -> (gmask, gchunks, record). record: per symbol block
    None (not retried) or a dict as retry_frame's."""
    e_max = CE.default_max_erasures(geo) if max_erasures is None or max_erasures < 0 else int(max_erasures)
    bpc = geo.CHUNK // geo.RS_DATA
    sym_chunks = geo.SYM_BLOCKS // bpc
    sym_mask = (1 << sym_chunks) - 1
    p = geo.RS_PARITY
    out = np.array(gchunks, np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    mmask = 0
    for m in member_masks:
        mmask |= int(m)
    blocks = stream_bytes(geo, np.asarray(cells) & 15)
    cmask, ok = combined_symbol_mask(geo, blocks, rs_ok) if disputed else (0, [True] * geo.SYM_BLOCKS)
    assert cmask & ~int(gmask) == 0, "the combined decode delivered a symbol chunk the retry-off group mask lacks"
    missing = sym_mask & ~(cmask | mmask)
    record = [None] * geo.SYM_BLOCKS
    emask = 0
    if disputed and missing:
        keys = _stream_pairs(geo, np.asarray(margins, np.int64)).min(1).reshape(geo.SYM_BLOCKS, geo.RS_BLOCK)
        status, msgs = {}, {}
        for b in range(geo.SYM_BLOCKS):
            if not (missing >> (b // bpc)) & 1:
                continue
            er = [] if ok[b] else _group_select(keys[b], e_max, rules)
            st, msg = _retry_block(blocks[b], er, ok[b], p, rules)
            status[b], msgs[b] = st, msg
            record[b] = dict(status=st, erasures=er, ok=ok[b], scores=keys[b])
        emask = _chunks_from_blocks(geo, 0, out, missing, status, msgs, "all", True)
    for j in range(sym_chunks):
        if (cmask >> j) & 1 or (emask >> j) & 1:
            continue
        if (mmask >> j) & 1:
            c = next(c for c in range(len(member_masks)) if (int(member_masks[c]) >> j) & 1)
            out[j] = np.asarray(member_chunks[c], np.uint8).reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)[j]
        else:
            out[j] = 0
    return (int(gmask) | mmask | emask) & geo.FULL_MASK, out, record
