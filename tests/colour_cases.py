"""Colour-path inputs and independent references (numpy only) for tests/test_colour_casts.py and tests/test_gpu_colour_casts.py.

- `cast`: a camera colour model in integer arithmetic (3x3 channel mix and per-channel gain in 1/256 fixed point, a black offset, an optional
  gamma look-up table, saturating at 0 and 255), and `FAMILIES` of casts built from it.
- `design_payload`: frame payloads whose fountain headers steer CimbReader::init_ccm (CimbReader.cpp:169-267): the first-appearance order of the
  four colours, a colour seen in one header cell only, a colour never seen (no matrix), an all-zero id (no header at all).
- `best_color`: a float32 restatement of CimbDecoder::get_best_color (CimbDecoder.cpp:27-55,168-200; color_correction.h:64-68), vectorised.
- `ccm64`: init_ccm's matrix in float64 -- the header cells' undrifted means grouped by expected colour, the anchor white, desired^T . pinv(actual^T)
  with OpenCV's singular-value cut-off -- and `von_kries64`, the same for color_correction == 1.
"""
import numpy as np

from libcimbar_amd import framegen, geometry

FLT_EPS = float(np.finfo(np.float32).eps)
BEST_COLOR_FLOOR = 48.0

# Common.cpp: getColor4 (colour_mode 1), getColor4_old and getColor8_old (colour_mode 0, the legacy modes)
PALETTE_B = np.array([[0, 255, 0], [0, 255, 255], [255, 255, 0], [255, 0, 255]], np.int32)
PALETTE_4_OLD = np.array([[0, 255, 255], [255, 255, 0], [255, 0, 255], [0, 255, 0]], np.int32)
PALETTE_8_OLD = np.array([[0, 255, 255], [127, 127, 255], [255, 0, 255], [255, 65, 65], [255, 159, 0], [255, 255, 0], [255, 255, 255], [0, 255, 0]], np.int32)


def palette(mode):
    return PALETTE_8_OLD if mode == 8 else PALETTE_4_OLD if mode == 4 else PALETTE_B


# ---------------------------------------------------------------------------------------------- camera colour model
def cast(frame, mix, gain, black=(0, 0, 0), gamma=None):
    """out_c = sat(black_c + (sum_k round(256 gain_c mix_ck) x_k + 128) >> 8), then out = lut[out] when gamma is given; uint8 in, uint8 out"""
    m = np.rint(256.0 * np.asarray(gain, np.float64)[:, None] * np.asarray(mix, np.float64)).astype(np.int64)
    x = frame.reshape(-1, 3).astype(np.int64)
    y = ((x @ m.T + 128) >> 8) + np.asarray(black, np.int64)[None, :]
    y = np.clip(y, 0, 255).astype(np.uint8)
    if gamma is not None:
        lut = np.clip(np.rint(255.0 * (np.arange(256) / 255.0) ** gamma), 0, 255).astype(np.uint8)
        y = lut[y]
    return y.reshape(frame.shape)


def _mix(rng, cross):
    m = np.eye(3) + rng.uniform(0, cross, (3, 3)) * (1 - np.eye(3))
    return m


def anchor_centres(geo):
    """the three 4x4 blocks calculateWhite reads (CimbReader.cpp:55-86, dark): top-left corners (x, y)"""
    a = 30                                                                     # anchor size (GridConf.h), every mode built here
    tl, right, bottom = a - 2, geo.IMG_W - a - 2, geo.IMG_H - a - 2
    return [(tl, tl), (tl, bottom), (right, tl)]


def family_cast(name, seed, frame, geo):
    """one member of a cast family applied to `frame`"""
    rng = np.random.default_rng(seed)
    if name == "mild":                        # white balance: gains 0.8-1.2, small crosstalk
        return cast(frame, _mix(rng, 0.06), rng.uniform(0.8, 1.2, 3))
    if name == "strong":                      # one gain 0.3-0.5, crosstalk up to 0.3: the matrix gets negative entries
        g = rng.uniform(0.85, 1.15, 3)
        g[rng.integers(3)] = rng.uniform(0.3, 0.5)
        return cast(frame, _mix(rng, 0.3), g, black=rng.integers(0, 12, 3))
    if name == "dead":                        # one channel dead (0) or stuck (constant): a rank-deficient system
        c = int(rng.integers(3))
        mix = _mix(rng, 0.05)
        mix[c] = 0
        black = np.zeros(3, np.int64)
        black[c] = 0 if seed % 2 == 0 else int(rng.integers(60, 200))
        return cast(frame, mix, rng.uniform(0.8, 1.1, 3), black=black)
    if name == "overexposed":                 # gains near 2 and crosstalk into one channel: two palette colours clip together
        mix = _mix(rng, 0.05)
        c = int(rng.integers(3))
        mix[c, (c + 1) % 3] = rng.uniform(1.0, 1.4)
        return cast(frame, mix, rng.uniform(1.6, 2.2, 3), black=rng.integers(0, 30, 3))
    if name == "underexposed":                # the white falls below BEST_COLOR_FLOOR
        return cast(frame, _mix(rng, 0.08), rng.uniform(0.1, 0.17, 3), gamma=float(rng.uniform(0.9, 1.2)))
    if name == "black_anchors":               # the anchor centres read black: the white takes its floor (1, 1, 1)
        out = cast(frame, _mix(rng, 0.1), rng.uniform(0.7, 1.1, 3))
        for x, y in anchor_centres(geo):
            out[y - 2:y + 6, x - 2:x + 6] = 0
        return out
    if name == "lifted":                      # lifted blacks: the minimum of every cell exceeds 48
        return cast(frame, _mix(rng, 0.1), rng.uniform(0.55, 0.75, 3), black=rng.integers(55, 95, 3), gamma=float(rng.uniform(0.7, 1.0)))
    if name == "mono":                        # all three channels equal
        w = rng.uniform(0.2, 0.5, 3)
        return cast(frame, np.tile(w / w.sum(), (3, 1)), np.full(3, rng.uniform(0.8, 1.1)))
    raise ValueError(name)


FAMILIES = ("mild", "strong", "dead", "overexposed", "underexposed", "black_anchors", "lifted", "mono")
WELL_CONDITIONED = ("mild", "strong", "underexposed", "black_anchors", "lifted")


# ---------------------------------------------------------------------------------------------- headers (FountainMetadata.h:16-92)
def chunk_counts(geo):
    sym_chunks = geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)
    return sym_chunks, geo.CHUNKS_PER_FRAME // 3      # symbol-stream chunks, headers the colour stream carries (NHDR)


def next_id(cur, radio):
    n = cur + 1
    if n == radio:
        n += 1
    return n & 0xFFFF


def chunk_headers(hdr4, first_id, nchunks, chunk):
    """the 6-byte headers of `nchunks` consecutive fountain chunks, ids advanced the way update_metadata predicts them"""
    fs = hdr4[3] | (hdr4[2] << 8) | (hdr4[1] << 16) | ((hdr4[0] & 0x80) << 17)
    radio = 0xFFFFFFFF if fs % chunk == 0 else fs // chunk
    out, cur = [], first_id & 0xFFFF
    for _ in range(nchunks):
        out.append(list(hdr4) + [(cur >> 8) & 0xFF, cur & 0xFF])
        cur = next_id(cur, radio)
    return np.array(out, np.uint8)


def expected_colours(headers):
    """(NHDR, 6) headers of the colour chunks -> (NHDR * 24,) expected colour of each header cell, cell order q = 24 c + t"""
    b = headers.astype(np.int64)
    return np.stack([(b[:, t >> 2] >> (6 - 2 * (t & 3))) & 3 for t in range(24)], 1).reshape(-1)


def design_payload(n, seed, mode, hdr4, first_id):
    """synth_payload with every frame's chunk headers replaced: bytes 0-3 = hdr4, ids consecutive from first_id (per frame), skipping the
    radioactive id as update_metadata does, so that the prediction init_ccm works from matches the cells on the frame"""
    geo = geometry.for_mode(mode)
    p = framegen.synth_payload(n, seed=seed, mode=mode).numpy().reshape(n, geo.CHUNKS_PER_FRAME, geo.CHUNK).copy()
    p[:, :, :6] = chunk_headers(hdr4, first_id, geo.CHUNKS_PER_FRAME, geo.CHUNK)[None]
    return p.reshape(n, geo.FRAME_BYTES)


def _pairs_avoid(v, colour):
    return all(((v >> s) & 3) != colour for s in (0, 2, 4, 6))


def header_designs(mode):
    """name -> (hdr4, first_id, expected counts per colour). All 24 orders of first appearance; colour 3 in one header cell only; colour 3 in none
    (the radioactive id skips the one id of the four whose low bits are 3); a zero id (no header, no matrix)."""
    import itertools
    geo = geometry.for_mode(mode)
    sym_chunks, nhdr = chunk_counts(geo)
    out = {}

    def add(name, hdr4, first_id):
        h = chunk_headers(hdr4, first_id, geo.CHUNKS_PER_FRAME, geo.CHUNK)[sym_chunks:sym_chunks + nhdr]
        out[name] = (list(hdr4), first_id, np.bincount(expected_colours(h), minlength=4))

    for k, perm in enumerate(itertools.permutations(range(4))):
        b0 = (perm[0] << 6) | (perm[1] << 4) | (perm[2] << 2) | perm[3]
        add("order%d%d%d%d" % perm, [b0, 0x5A ^ (k * 7 & 0xFF), 0x3C, 0x81 ^ k], 0x0100 + 37 * k)
    # colour 3 once: bytes 0-3 and the id's high byte avoid it; the colour chunks' ids end at 0x43 (of 0x40..0x43 only 0x43 has a '3' pair)
    add("one_cell", [0x12, 0x21, 0x06, 0x18], 0x44 - nhdr - sym_chunks)
    # colour 3 never: colour-chunk ids j, j + 1, j + 2, (j + 3 is the radioactive id) j + 4, none with a '3' pair; a file size fs with
    # fs // chunk == j + 3 and no '3' pair in its bytes
    def absent():
        for j in range(0x40, 0x10000, 0x40):
            if not all(_pairs_avoid(v >> 8, 3) and _pairs_avoid(v & 0xFF, 3) for v in (j, j + 1, j + 2, j + 4)):
                continue
            for fs in range((j + 3) * geo.CHUNK + 1, (j + 4) * geo.CHUNK):
                b = [(fs >> 17) & 0x80 | 0x12, (fs >> 16) & 0xFF, (fs >> 8) & 0xFF, fs & 0xFF]
                if (fs >> 25) == 0 and all(_pairs_avoid(v, 3) for v in b):
                    return b, j - sym_chunks
    add("absent", *absent())
    add("zero_id", [0, 0, 0, 0], 0x40)
    assert out["one_cell"][2][3] == 1 and out["absent"][2][3] == 0 and (out["absent"][2][:3] > 0).all(), out
    for k in out:
        if k.startswith("order"):
            assert (out[k][2] > 0).all()
    return out


# ---------------------------------------------------------------------------------------------- classifier (CimbDecoder.cpp:168-200)
def _transformed(rgb, m):
    f32 = np.float32
    r, g, b = (np.ascontiguousarray(rgb[:, k], dtype=f32) for k in range(3))
    if m is not None:
        m = np.asarray(m, f32)
        # Matx33f * Matx31f (color_correction.h:64-68): s = 0; s += m(i, k) * v(k) for k = 0, 1, 2 -- every step rounded to float
        r, g, b = [((f32(0) + m[3 * i] * r) + m[3 * i + 1] * g) + m[3 * i + 2] * b for i in range(3)]
    return r, g, b


def _fixed(r, g, b):
    """max / min with 1.0 and BEST_COLOR_FLOOR, adjust = 255.0 / (max - min) in double narrowed to float, fix_single_color (CimbDecoder.cpp:27-36,
    176-182) -> three int32 channels"""
    f32 = np.float32
    mx = np.maximum(np.maximum(np.maximum(r, g), b), f32(1.0))
    mn = np.minimum(np.minimum(np.minimum(r, g), b), f32(BEST_COLOR_FLOOR))
    mn = np.where(mn >= mx, f32(0), mn)
    adjust = (255.0 / (mx - mn).astype(np.float64)).astype(f32)
    hi = f32(245) - mn
    out = []
    for c in (r, g, b):
        c = (c - mn) * adjust
        c = np.where(c > hi, f32(255), c)
        c = np.where(c < 0, f32(0), c)
        out.append(c.astype(np.int32) & 0xFF)                                # (uchar)c: truncation (c is never negative here)
    return out


def _distances(c0, c1, c2, pal):
    rel = (c0 - c1, c1 - c2, c2 - c0)
    for p in pal:
        q = (int(p[0]) - int(p[1]), int(p[1]) - int(p[2]), int(p[2]) - int(p[0]))
        yield (rel[0] - q[0]) ** 2 + (rel[1] - q[1]) ** 2 + (rel[2] - q[2]) ** 2


def best_color(rgb, m=None, pal=PALETTE_B):
    """rgb (N, 3) values exactly representable in float32; m = 9 float32 (row-major Matx33f) or None (no active matrix) -> (N,) uint8:
    CimbDecoder::get_best_color, squared distance of the relative colours, first minimum wins (distance < best_distance)"""
    c0, c1, c2 = _fixed(*_transformed(rgb, m))
    best = np.zeros(len(c0), np.uint8)
    best_d = None
    for i, d in enumerate(_distances(c0, c1, c2, pal)):
        if best_d is None:
            best_d = d
            continue
        take = d < best_d
        best[take] = i
        best_d = np.where(take, d, best_d)
    return best


def tie_margin(rgb, m=None, pal=PALETTE_B):
    """second-smallest minus smallest squared distance (0: a tie that the first-minimum rule decides)"""
    c0, c1, c2 = _fixed(*_transformed(rgb, m))
    d = np.sort(np.stack(list(_distances(c0, c1, c2, pal)), 1), 1)
    return d[:, 1] - d[:, 0]


def near_tie(rgb, m=None, pal=PALETTE_B):
    """cells whose class changes when one channel of the mean moves by one unit"""
    base = best_color(rgb, m, pal)
    out = np.zeros(len(rgb), bool)
    for k in range(3):
        for dv in (-1, 1):
            x = rgb.copy()
            x[:, k] = np.clip(x[:, k] + dv, 0, 255)
            out |= best_color(x, m, pal) != base
    return out


def all_rgb(lo=0, hi=1 << 24):
    """integer RGB triples lo..hi-1 (r = bits 16-23, g = 8-15, b = 0-7) as float32 (N, 3)"""
    v = np.arange(lo, hi, dtype=np.uint32)
    return np.stack([(v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF], 1).astype(np.float32)


def stratified_rgb(n_bits=20, seed=0):
    """2^n_bits integer RGB: one uniform draw from each of the 2^n_bits equal cells of the cube"""
    rng = np.random.default_rng(seed)
    k = n_bits // 3
    side = 256 >> k
    idx = np.arange(1 << (3 * k))
    base = np.stack([(idx >> (2 * k)) & ((1 << k) - 1), (idx >> k) & ((1 << k) - 1), idx & ((1 << k) - 1)], 1) * side
    pts = base + rng.integers(0, side, base.shape)
    extra = rng.integers(0, 256, ((1 << n_bits) - len(pts), 3))
    return np.concatenate([pts, extra]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- float64 CCM
def header_cells(geo):
    """(NHDR * 24,) linear cell index of the header cells: colour-stream cell interval * c + t (CimbReader.cpp:188-227)"""
    ncol = geo.NCELLS                                                          # colour stream: one 2-bit field per cell
    interval = (geo.NCELLS * 6 // 8) * 8 // geo.CHUNKS_PER_FRAME // 2
    idx = geo.interleave_indices()
    stream = [s for block in range(0, ncol, interval) for s in range(block, block + 24)]
    return idx[np.array(stream)]


def cell_means(frame, geo, cells):
    """Cell.h:30-62 mean_rgb over the 6x6 inside each undrifted cell: uint16 sums / 36"""
    xy = geo.cell_positions()[cells] + 1
    out = np.empty((len(cells), 3), np.int64)
    for k, (x, y) in enumerate(xy):
        out[k] = (frame[y:y + 6, x:x + 6].reshape(-1, 3).astype(np.int64).sum(0) & 0xFFFF) // 36
    return out


def white64(frame, geo):
    """calculateWhite (dark): channel-wise max of the three 4x4 anchor-centre means, floor 1"""
    w = np.ones(3)
    for x, y in anchor_centres(geo):
        w = np.maximum(w, frame[y:y + 4, x:x + 4].reshape(-1, 3).astype(np.float64).mean(0))
    return w


def ccm_system(frame, geo, colour_headers):
    """(actual (R, 3), desired (R, 3)) of init_ccm, or None where it bails (fewer than four colours)"""
    exp = expected_colours(colour_headers)
    means = cell_means(frame, geo, header_cells(geo))
    pal = palette(geo.MODE)
    actual, desired = [], []
    for c in range(4):
        sel = exp == c
        if not sel.any():
            return None
        actual.append(means[sel].sum(0) // sel.sum())                          # unsigned sums / count, CimbReader.cpp:241-243
        desired.append(pal[c])
    actual.append(white64(frame, geo))
    desired.append([255, 255, 255])
    return np.array(actual, np.float64), np.array(desired, np.float64)


def pinv_cut(y):
    """pinv(y) through the SVD, dropping singular values W_i <= 2 FLT_EPSILON sum(W) (cv::invert(DECOMP_SVD), lapack.cpp SVBkSb); also
    returns the singular values and the cut-off"""
    u, s, vt = np.linalg.svd(y, full_matrices=False)
    thr = 2 * FLT_EPS * s.sum()
    inv = np.where(s > thr, 1.0 / np.where(s > 0, s, 1.0), 0.0)
    return (vt.T * inv) @ u.T, s, thr


def ccm64(actual, desired):
    """desired^T . pinv(actual^T) in float64 -> (ccm (3, 3), singular values, cut-off)"""
    p, s, thr = pinv_cut(actual.T)
    return desired.T @ p, s, thr


VK_T = np.array([[0.40024, 0.7076, -0.08081], [-0.2263, 1.16532, 0.0457], [0.0, 0.0, 0.91822]])


def von_kries64(white):
    """get_adaptation_matrix<von_kries>(white, (255, 255, 255)) in float64: T^-1 diag(T 255 / T white) T"""
    T = VK_T.astype(np.float32).astype(np.float64)
    d = np.diag((T @ np.full(3, 255.0)) / (T @ np.asarray(white, np.float64)))
    return np.linalg.inv(T) @ d @ T


def ccm_bound(c64, s, thr, c=16.0):
    """|ccm32 - ccm64| <= c kappa 2^-23 |ccm64| elementwise, kappa over the singular values kept. None (skip) where a singular value lies within 10x
    of the cut-off, or below it without being exactly zero: in float32 such a value is rounding noise of the cut-off's own size (a monochrome
    camera's two missing directions), so which side of the cut-off the Jacobi SVD puts it on is not a property of the exact system. An exactly
    zero one (a dead channel) is dropped by both."""
    if ((s > 0) & (s < thr * 10)).any():
        return None
    kept = s[s > thr]
    kappa = kept.max() / kept.min()
    return c * kappa * 2.0 ** -23 * np.abs(c64).max()
