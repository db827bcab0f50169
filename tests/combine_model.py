"""A numpy restatement of multi-capture decoding's grouping and combined cells (include/cimbar_hip.h, cimbar_hip_decode_batch_combined;
csrc/combine.hip.inc k_group_agree / k_group_walk / k_group_cells), written from the rule rather than from the kernels.

group_captures(symbols, colors, usable, min_agree_permille, max_group, groups_in) -> groups (n,) int32, -1 = in no group
    raises ValueError where the library returns CIMBAR_HIP_EINVAL (max_group above 8, an invalid groups_in)
combine_cells(mode, bitplanes, symbols, colors, drift, flood_path, members) -> (cells (NCELLS,) uint8 colour << 4 | symbol,
                                                                              margins (NCELLS,) uint16, 0xFFFF = symbol not disputed)
    from the per-capture taps of the members' batch (TAP_BITPLANE, TAP_SYMBOLS, TAP_COLORS, TAP_DRIFT, TAP_FLOOD_PATH), members = the
    capture indices of one group in capture order
"""
import numpy as np

from libcimbar_amd import geometry, modeb

GMAX = 8
MARGIN_NONE = 0xFFFF


def agree(symbols, colors):
    """(n - 1,) cells whose symbol and colour are both equal in captures k and k + 1"""
    s, c = np.asarray(symbols), np.asarray(colors)
    return ((s[1:] == s[:-1]) & (c[1:] == c[:-1])).sum(axis=1)


def resolve(min_agree_permille, max_group):
    if max_group > GMAX:
        raise ValueError("max_group above 8")
    return (750 if min_agree_permille <= 0 else min_agree_permille), (4 if max_group <= 0 else max_group)


def check_groups_in(groups_in, max_group):
    """-1 or an id; ids start at 0 and rise by one; each id's captures contiguous and at most max_group"""
    nxt, cur, cnt = 0, -1, 0
    for v in (int(x) for x in groups_in):
        if v == -1:
            cur = -1
        elif v == cur:
            cnt += 1
            if cnt > max_group:
                raise ValueError("a group of more than max_group captures")
        elif v == nxt:
            cur, cnt, nxt = v, 1, nxt + 1
        else:
            raise ValueError("ids must be -1 or start at 0, rise by one and be contiguous")


def group_captures(symbols, colors, usable=None, min_agree_permille=0, max_group=0, groups_in=None):
    n = len(symbols)
    ncells = np.asarray(symbols).shape[1]
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    min_agree, max_group = resolve(min_agree_permille, max_group)
    out = np.full(n, -1, np.int32)
    if groups_in is not None:
        check_groups_in(groups_in, max_group)
        for k in range(n):
            out[k] = int(groups_in[k]) if usable[k] else -1
        return out
    a = agree(symbols, colors) if n > 1 else np.zeros(0, np.int64)
    gid, size = -1, 0
    for k in range(n):
        if not usable[k]:
            continue
        new = (k == 0 or not usable[k - 1] or int(a[k - 1]) * 1000 < min_agree * ncells or size >= max_group)
        if new:
            gid, size = gid + 1, 0
        out[k] = gid
        size += 1
    return out


def n_groups(groups):
    return int(np.max(groups)) + 1 if len(groups) and np.max(groups) >= 0 else 0


def members(groups, g):
    return [k for k in range(len(groups)) if groups[k] == g]


def cell_hashes(mode, bitplane, drift, flooded):
    """(NCELLS,) uint64: each cell's 8x8 hash at its final position (cell_xy + drift where the capture took the flood pass) from one capture's
    TAP_BITPLANE bytes (bit x + IMG_W * y, MSB first); bit 63 = top-left pixel"""
    geo = geometry.for_mode(mode)
    bits = np.unpackbits(np.asarray(bitplane, np.uint8)).reshape(geo.IMG_H, geo.IMG_W)
    xy = geo.cell_positions().astype(np.int64)
    if flooded:
        xy = xy + np.asarray(drift, np.int64).reshape(-1, 2)
    rows = xy[:, 1, None] + np.arange(8)[None, :]
    cols = xy[:, 0, None] + np.arange(8)[None, :]
    block = bits[rows[:, :, None], cols[:, None, :]]                          # (NCELLS, 8, 8)
    packed = np.packbits(block.reshape(len(xy), 64), axis=1)                 # 8 bytes per cell, first row first
    return packed.view(">u8").reshape(-1).astype(np.uint64)


def _popcount64(x):
    x = np.asarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def combine_cells(mode, bitplanes, symbols, colors, drift, flood_path, member_list, tiles=None):
    tiles = modeb.TILE_HASHES if tiles is None else np.asarray(tiles, np.uint64)
    m = len(member_list)
    ncells = np.asarray(symbols).shape[1]
    S = np.stack([np.asarray(symbols[c], np.int64) & 15 for c in member_list])          # (m, NCELLS)
    C = np.stack([np.asarray(colors[c], np.int64) for c in member_list])
    cells = np.zeros(ncells, np.uint8)
    margins = np.full(ncells, MARGIN_NONE, np.uint16)
    if m == 0:
        return cells, margins
    H = np.stack([cell_hashes(mode, bitplanes[c], drift[c], flood_path[c] != 0) for c in member_list])   # (m, NCELLS)
    D = _popcount64(H[:, :, None] ^ tiles[None, None, :])                                               # (m, NCELLS, 16): d_c(t)
    for i in range(ncells):
        s, col, d = S[:, i], C[:, i], D[:, i, :]
        if (s == s[0]).all():
            shat = int(s[0])
        else:
            score = [int(sum(2 * d[c, t] - (1 if s[c] == t else 0) for c in range(m))) for t in range(16)]
            shat = min(range(16), key=lambda t: (score[t], t))
            rest = sorted(score[t] for t in range(16) if t != shat)
            margins[i] = rest[0] - score[shat]
        votes = {v: int((col == v).sum()) for v in set(col.tolist())}
        top = max(votes.values())
        tied = [v for v in votes if votes[v] == top]
        if len(tied) == 1:
            ccol = tied[0]
        else:
            best = min((c for c in range(m) if col[c] in tied), key=lambda c: (int(d[c, shat]), c))
            ccol = int(col[best])
        cells[i] = (ccol << 4) | shat
    return cells, margins
