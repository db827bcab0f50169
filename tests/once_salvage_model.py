"""Tear salvage restated in numpy from the wording of include/cimbar_hip.h ("Tear salvage"): a torn candidate's two sides and their line
ranges, the partials of a run, which runs qualify and which are tried, the order of a tried run's group, the word
CIMBAR_HIP_TAP_ONCE_SALVAGE reports per run slot, and the combined cells where a partial takes part in some cells only. Nothing here comes
from the kernel side. The tear records, runs, lists and roles are tests/once_tear_model.py's and tests/repeat_skip_model.py's; a cell's hash
is tests/combine_model.cell_hashes'; a tried run's row is tests/once_rescue_model.compose_row over the FULL members."""
import numpy as np

from libcimbar_amd import geometry, modeb
from tests import combine_model as CM
from tests import once_tear_model as OT
from tests import repeat_skip_model as RM

GMAX = 8
GUARD_DEFAULT, GUARD_MAX = 1, 16
NO_PARTIAL = (-1, -1, 0, 0)


def resolve(guard_lines=-1):
    """-1 resolves to 1; 0 .. 16 are legal; anything else is refused (ValueError where the library returns CIMBAR_HIP_EINVAL)"""
    if guard_lines == -1:
        return GUARD_DEFAULT
    if not 0 <= guard_lines <= GUARD_MAX:
        raise ValueError("guard_lines must be -1 or 0 .. 16")
    return guard_lines


def effective(on, rescue_on, tear_axis, want_rchunks, want_rmasks):
    return bool(on) and bool(rescue_on) and tear_axis != -1 and (want_rchunks or want_rmasks)


# ------------------------------------------------------------------------------------------------ sides
def sides(mode, rec, guard):
    """(P side, N side) of a candidate with the record {w, s, first, last}: each (axis, lo, hi), or None where the range is empty.
    low = [0, s - g), high = [s + g, L); the P side is low when o = 0 and high when o = 1"""
    w, s = int(rec[0]), int(rec[1])
    assert w >= 0, "no candidate"
    axis, o = w >> 1, w & 1
    L = OT.lines(mode, axis)[1]
    low, high = (0, s - guard), (s + guard, L)
    keep = lambda r: (axis, r[0], r[1]) if r[0] < r[1] else None
    return (keep(low), keep(high)) if o == 0 else (keep(high), keep(low))


def is_fallback_candidate(k, n, rec, roles):
    return 0 <= k < n and int(rec[k][0]) >= 0 and int(roles[k]) == RM.FALLBACK


def partials(mode, members, rec, roles, guard):
    """per run (preceding, following): each (capture, axis, lo, hi) or None. A candidate's own run has neither."""
    n = len(rec)
    out = []
    for m in members:
        if len(m) == 1 and int(rec[m[0]][0]) >= 0:
            out.append((None, None))
            continue
        f, e = m[0], m[-1]
        prec = foll = None
        if is_fallback_candidate(f - 1, n, rec, roles):
            side = sides(mode, rec[f - 1], guard)[1]           # its N side: where it agreed with the capture behind it, f
            prec = (f - 1,) + side if side else None
        if is_fallback_candidate(e + 1, n, rec, roles):
            side = sides(mode, rec[e + 1], guard)[0]           # its P side: where it agreed with the capture in front of it, e
            foll = (e + 1,) + side if side else None
        out.append((prec, foll))
    return out


# ------------------------------------------------------------------------------------------------ qualifies, tried, the group
def qualifies(mode, members, rec, masks, parts):
    """per run: no candidate's run, the representative's mask is not full, and the run has two members or a partial"""
    full = geometry.for_mode(mode).FULL_MASK
    out = []
    for m, (prec, foll) in zip(members, parts):
        cand = len(m) == 1 and int(rec[m[0]][0]) >= 0
        out.append(not cand and int(masks[RM.representative(m)]) != full and (len(m) >= 2 or prec is not None or foll is not None))
    return out


def tried(mode, members, rec, masks, parts):
    """qualifies, and the OR of the full members' masks after pass 2 is not full"""
    full = geometry.for_mode(mode).FULL_MASK
    out = []
    for m, q in zip(members, qualifies(mode, members, rec, masks, parts)):
        union = 0
        for k in m:
            union |= int(masks[k])
        out.append(q and union != full)
    return out


def group(m, part):
    """the group of a tried run: [(capture, None)] for the full members in capture order, then the preceding and the following partial as
    (capture, (axis, lo, hi)), each only while the group has fewer than GMAX members"""
    g = [(k, None) for k in m]
    for p in part:
        if p is not None and len(g) < GMAX:
            g.append((p[0], tuple(p[1:])))
    return g


def tap_rows(n, members, tried_runs, parts):
    """(n, 8) int32, CIMBAR_HIP_TAP_ONCE_SALVAGE: per run slot {kp, axis_p, lo_p, hi_p, kf, axis_f, lo_f, hi_f}; NO_PARTIAL for a partial the
    run's group does not have, for a run that is not tried and for the slots at and above the run count"""
    out = np.tile(np.array(NO_PARTIAL + NO_PARTIAL, np.int32), (n, 1))
    for r, (m, t, part) in enumerate(zip(members, tried_runs, parts)):
        if not t:
            continue
        joined = [k for k, rng in group(m, part) if rng is not None]      # (the cap may have kept a partial out)
        for h, p in enumerate(part):
            if p is not None and p[0] in joined:
                out[r, 4 * h:4 * h + 4] = p
    return out


# ------------------------------------------------------------------------------------------------ combined cells with participation
def participation(mode, grp):
    """(members, NCELLS) bool: a full member takes part in every cell, a partial in cell i iff lo <= line_axis(i) < hi"""
    ncells = geometry.for_mode(mode).NCELLS
    out = np.ones((len(grp), ncells), bool)
    for c, (_, rng) in enumerate(grp):
        if rng is not None:
            axis, lo, hi = rng
            line = OT.lines(mode, axis)[0]
            out[c] = (line >= lo) & (line < hi)
    return out


def combine_cells(mode, bitplanes, symbols, colors, drift, flood_path, grp, tiles=None):
    """the combined calls' rule per cell over that cell's participants -> (cells colour << 4 | symbol, margins, disputed: whether the
    participants of any cell differ). The per-capture arrays are indexed by the captures named in grp (dicts or arrays)."""
    tiles = modeb.TILE_HASHES if tiles is None else np.asarray(tiles, np.uint64)
    caps = [k for k, _ in grp]
    m = len(caps)
    assert m >= 1 and grp[0][1] is None, "member 0 is always a full member"
    S = np.stack([np.asarray(symbols[k], np.int64) & 15 for k in caps])
    C = np.stack([np.asarray(colors[k], np.int64) for k in caps])
    ncells = S.shape[1]
    who = participation(mode, grp)
    H = np.stack([CM.cell_hashes(mode, bitplanes[k], drift[k], flood_path[k] != 0) for k in caps])
    cells = np.zeros(ncells, np.uint8)
    margins = np.full(ncells, CM.MARGIN_NONE, np.uint16)
    disputed = False
    for i in range(ncells):
        idx = np.flatnonzero(who[:, i])                       # positions in the group's order
        s, col = S[idx, i], C[idx, i]
        if (s == s[0]).all() and (col == col[0]).all():
            cells[i] = (int(col[0]) << 4) | int(s[0])
            continue
        disputed = True
        d = CM._popcount64(H[idx, i, None] ^ tiles[None, :])  # (participants, 16)
        if (s == s[0]).all():
            shat = int(s[0])
        else:
            score = [int(sum(2 * d[c, t] - (1 if s[c] == t else 0) for c in range(len(idx)))) for t in range(16)]
            shat = min(range(16), key=lambda t: (score[t], t))
            margins[i] = sorted(score[t] for t in range(16) if t != shat)[0] - score[shat]
        votes = {v: int((col == v).sum()) for v in set(col.tolist())}
        top = max(votes.values())
        tied = [v for v in votes if votes[v] == top]
        if len(tied) == 1:
            ccol = tied[0]
        else:
            best = min((c for c in range(len(idx)) if col[c] in tied), key=lambda c: (int(d[c, shat]), c))
            ccol = int(col[best])
        cells[i] = (ccol << 4) | shat
    return cells, margins, disputed
