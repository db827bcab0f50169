"""The capture blur (k_scan_gray_blur_rows / k_scan_gray_blur + k_scan_otsu) at the places where the two kernels are partitioned: the case
table of tests/test_gpu_scan_blur.py, vetted without a GPU by tests/test_scan_blur_cases.py.

    partition(w, h)     launch_gray_blur's choice restated: streaming or tiled, blur unit, column blocks / strips or tiles and what is left
                        over in the last of each
    gray_blur(rgb)      the operation restated in numpy integers (RGB2GRAY, separable fixed-point Gaussian, one rounding, reflect-101)
    otsu(hist, w, h)    getThreshVal_Otsu_8u in Python doubles, in the reference's order
    capture(case)       the capture bytes of a case and the RGB image the oracle's co_capture_to_rgb makes of them
    reference(case)     co_gray_blur's plane and histogram and co_scan_preprocess's threshold, computed once per case and kept read-only
    FAULTS              six wrong results a partitioning mistake would produce, planted into a reference result"""
import collections
import functools

import numpy as np

from oracle import pyref
from oracle.pyref import P
from tests import capture_formats as CF

X1S_ROWS, X1_TW, X1_TH, X1_TILES, LANES_MAX = 30, 128, 32, 4, 62     # extract.hip.inc / launch_gray_blur

Case = collections.namedtuple("Case", "name w h n fmt seed content")


def _c(name, w, h, n=1, fmt=3, seed=None, content="noise"):
    return Case(name, w, h, n, fmt, seed if seed is not None else w * 7919 + h + fmt, content)


STREAMING_3 = [_c("16x8", 16, 8), _c("32x31", 32, 31), _c("992x30", 992, 30), _c("1008x121", 1008, 121), _c("1024x119", 1024, 119),
               _c("1984x62", 1984, 62), _c("2000x60", 2000, 60)]
STREAMING_5 = [_c("1504x1500", 1504, 1500), _c("2000x1501", 2000, 1501), _c("1984x1502", 1984, 1502), _c("1520x1529", 1520, 1529)]
TILED = [_c("8x8", 8, 8), _c("129x33", 129, 33), _c("127x129", 127, 129), _c("130x40", 130, 40), _c("132x40", 132, 40),
         _c("1501x1500", 1501, 1500), _c("2561x2529", 2561, 2529), _c("4609x4500", 4609, 4500)]
FORMATS = [_c(f"{w}x{h}-fmt{fmt}", w, h, fmt=fmt) for (w, h) in ((1008, 122), (130, 40)) for fmt in CF.FORMATS]
BATCHES = [_c("131x37-n3", 131, 37, n=3), _c("32x31-n3", 32, 31, n=3)]
DEGENERATE = [_c("flat0", 64, 40, content="flat0"), _c("flat100", 64, 40, content="flat100"), _c("flat255", 64, 40, content="flat255"),
              _c("halves", 64, 40, content="halves"), _c("one-white-4000x2600", 4000, 2600, content="one_white")]
CASES = STREAMING_3 + STREAMING_5 + TILED + FORMATS + BATCHES + DEGENERATE
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# an RGB capture in device memory this many bytes behind a 16-byte boundary: launch_gray_blur must leave the streaming kernel for the tiled
# RGB one, which then stages every row with a non-zero offset
MISALIGNED = BY_NAME["1008x121"]
MISALIGNED_OFFSETS = (1, 4)
# the two cases whose tapped plane is also held against cimbar_hip_scan_preprocess (one per kernel)
PREPROCESS_TIE = ("1008x121", "129x33")
HALVES_LEVELS = (100, 101)
ONE_WHITE_THRESHOLD = 4     # what the oracle gives for one-white-4000x2600 (1 / (w h) < FLT_EPSILON: the top bin alone is skipped)


def blur_unit(w, h):
    """Scanner.h:157-159: max(3, nextPowerOfTwo(min(w, h) * 0.002) + 1), in the 32-bit arithmetic of the C code"""
    v = (int(min(w, h) * 0.002) - 1) & 0xFFFFFFFF
    for s in (1, 2, 4, 8, 16):
        v |= v >> s
    v = (v + 2) & 0xFFFFFFFF
    return v if v > 3 else 3


def partition(w, h, aligned=True):
    """How launch_gray_blur cuts a w x h capture up (aligned: the capture and the output plane start on 16-byte boundaries)"""
    unit = blur_unit(w, h)
    p = {"w": w, "h": h, "unit": unit, "radius": unit // 2}
    if unit <= 5 and w % 16 == 0 and aligned:
        groups = w // 16
        nb = (groups + LANES_MAX - 1) // LANES_MAX
        lanes_out = (groups + nb - 1) // nb
        strips = (h + X1S_ROWS - 1) // X1S_ROWS
        p.update(kernel="streaming", groups=groups, nb=nb, lanes_out=lanes_out,
                 block_groups=[min(lanes_out, groups - b * lanes_out) for b in range(nb)],
                 strips=strips, last_strip_rows=h - (strips - 1) * X1S_ROWS, workgroups_y=(strips + 3) // 4,
                 ring_rows=unit, unroll=3 if unit == 3 else 10)
    else:
        tiles_x, tiles_y = (w + X1_TW - 1) // X1_TW, (h + X1_TH - 1) // X1_TH
        p.update(kernel="tiled", tiles_x=tiles_x, last_tile_cols=w - (tiles_x - 1) * X1_TW, tiles_y=tiles_y,
                 last_tile_rows=h - (tiles_y - 1) * X1_TH, workgroups_y=(tiles_y + X1_TILES - 1) // X1_TILES,
                 stores="dword" if w % 4 == 0 else "byte", frame_bytes_mod16=(w * h * 3) % 16)
    return p


K = {3: [1, 2, 1], 5: [1, 4, 6, 4, 1], 9: [4, 13, 30, 51, 60, 51, 30, 13, 4], 17: [1, 2, 4, 8, 13, 21, 28, 33, 36, 33, 28, 21, 13, 8, 4, 2, 1]}
SHIFT = {3: 4, 5: 8, 9: 16, 17: 16}


def gray_of(rgb):
    rgb = rgb.astype(np.int32)
    return ((rgb[..., 0] * 9798 + rgb[..., 1] * 19235 + rgb[..., 2] * 3735 + (1 << 14)) >> 15).astype(np.int32)


def gray_blur(rgb, border="reflect"):
    """(h, w, 3) uint8 -> (plane (h, w) uint8, histogram (256,) int64). border: numpy's "reflect" is BORDER_REFLECT_101; "edge" (replicate)
    is what the planted faults use"""
    h, w = rgb.shape[:2]
    unit = blur_unit(w, h)
    k, r = K[unit], unit // 2
    g = np.pad(gray_of(rgb), ((0, 0), (r, r)), mode=border)
    hs = np.zeros((h, w), np.int32)
    for t, kt in enumerate(k):
        hs += kt * g[:, t:t + w]
    del g
    hs = np.pad(hs, ((r, r), (0, 0)), mode=border)
    acc = np.zeros((h, w), np.int32)
    for t, kt in enumerate(k):
        acc += kt * hs[t:t + h]
    out = ((acc + (1 << (SHIFT[unit] - 1))) >> SHIFT[unit]).astype(np.uint8)
    return out, np.bincount(out.reshape(-1), minlength=256)


FLT_EPSILON = float(np.finfo(np.float32).eps)


def otsu(hist, w, h):
    """thresh.cpp getThreshVal_Otsu_8u: Python floats are the doubles of the C code, the operations are in its order"""
    scale = 1.0 / (float(w) * float(h))
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p_i = float(hist[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def capture(case):
    """-> (captures (n, bytes) uint8 in the case's format, rgb (n, h, w, 3) uint8: co_capture_to_rgb of each)"""
    w, h, n, fmt = case.w, case.h, case.n, case.fmt
    nbytes = CF.capture_bytes(w, h, fmt)
    if case.content == "noise":
        # noise with a darker top half, so that Otsu has something to find (other formats: the first half of the plane that carries luma)
        buf = np.random.default_rng(case.seed).integers(0, 256, (n, nbytes), dtype=np.uint8)
        buf[:, : w * (h // 2) * {3: 3, 4: 4}.get(fmt, 1)] //= 3
    else:
        assert fmt == 3
        img = np.zeros((n, h, w, 3), np.uint8)
        if case.content.startswith("flat"):
            img[:] = int(case.content[4:])
        elif case.content == "halves":
            # two neighbouring levels, w h / 2 pixels each: the [1 2 1] blur rounds the seam's a + 1/4 and a + 3/4 back to a and a + 1, so
            # the histogram has exactly two bins of equal weight and q1 = q2 = 1/2
            img[:, :, : w // 2] = HALVES_LEVELS[0]
            img[:, :, w // 2:] = HALVES_LEVELS[1]
        elif case.content == "one_white":
            img[:, h // 2, w // 2] = 255
        buf = img.reshape(n, nbytes)
    buf = np.ascontiguousarray(buf)
    if fmt == 3:
        return buf, buf.reshape(n, h, w, 3)
    rgb = np.zeros((n, h, w, 3), np.uint8)
    L = pyref.oracle_lib()
    for k in range(n):
        assert L.co_capture_to_rgb(P(buf[k]), w, h, fmt, P(rgb[k])) == 0
    return buf, rgb


def oracle_result(rgb):
    """(h, w, 3) uint8 -> (co_gray_blur's plane, its histogram as int64, co_scan_preprocess's threshold)"""
    L = pyref.oracle_lib()
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    gray, hist, binary = np.zeros((h, w), np.uint8), np.zeros(256, np.int32), np.zeros((h, w), np.uint8)
    assert L.co_gray_blur(P(rgb), w, h, P(gray), P(hist)) == blur_unit(w, h)
    thr = L.co_scan_preprocess(P(rgb), w, h, P(binary))
    assert thr >= 0
    return gray, hist.astype(np.int64), thr


@functools.lru_cache(maxsize=4)
def reference(name):
    """-> (captures, gray (n, h, w), hist (n, 256), thr (n,)) of a case, read-only. Only the last few are kept: the large cases hold 60 MB each"""
    case = BY_NAME[name]
    buf, rgb = capture(case)
    res = [oracle_result(rgb[k]) for k in range(case.n)]
    out = (buf, np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- planted faults
# Each takes (rgb, gray, hist) of one capture -- the reference result -- and returns a wrong (gray, hist). A kernel builds its histogram from the
# values it stores, so a fault in the plane carries over into the histogram; the one histogram fault leaves the plane alone.
def _with_hist(gray):
    return gray, np.bincount(gray.reshape(-1), minlength=256)


def fault_repeated_row(rgb, gray, hist):
    """the first row of the second strip repeats the row above: a wrong ring slot at a strip boundary"""
    g = gray.copy()
    g[X1S_ROWS] = g[X1S_ROWS - 1]
    return _with_hist(g)


def fault_corner_group(rgb, gray, hist):
    """replicate instead of reflect-101 in the top-left 16-pixel group of the first strip: a wrong halo at an image corner"""
    g = gray.copy()
    wrong = gray_blur(rgb, "edge")[0]
    g[:X1S_ROWS, :16] = wrong[:X1S_ROWS, :16]
    return _with_hist(g)


def fault_column_seam(rgb, gray, hist):
    """+1 on the first column of the second column block"""
    g = gray.copy()
    p = partition(gray.shape[1], gray.shape[0])
    x = p["lanes_out"] * 16 if p["kernel"] == "streaming" and p["nb"] > 1 else X1_TW
    g[:, x] = np.minimum(g[:, x].astype(np.int32) + 1, 255).astype(np.uint8)
    return _with_hist(g)


def fault_hist_16(rgb, gray, hist):
    """the histogram loses 16 counts in its fullest bin: the streaming kernel's "flat group adds 16" shortcut gone wrong"""
    hs = hist.copy()
    hs[int(np.argmax(hs))] -= 16
    return gray, hs


def fault_first_column(rgb, gray, hist):
    """replicate instead of reflect-101 on the whole first column"""
    g = gray.copy()
    g[:, 0] = gray_blur(rgb, "edge")[0][:, 0]
    return _with_hist(g)


def fault_last_row(rgb, gray, hist):
    """replicate instead of reflect-101 on the whole last row"""
    g = gray.copy()
    g[-1] = gray_blur(rgb, "edge")[0][-1]
    return _with_hist(g)


# fault -> the case it is planted into: one with a second strip, a second column block and a dark top-left corner
FAULTS = {"repeated_row": fault_repeated_row, "corner_group": fault_corner_group, "column_seam": fault_column_seam, "hist_16": fault_hist_16,
          "first_column": fault_first_column, "last_row": fault_last_row}
FAULT_CASE = "1008x121"
# the faults the comparison of binary image + threshold (tests/test_gpu_extract.py, tests/test_gpu_capture_formats.py) cannot see on that case
MUST_ESCAPE_BINARY = ("repeated_row", "corner_group", "hist_16")


def differences(got, want, limit=6):
    """the first few coordinates at which two planes differ, for a failure message: [(frame, y, x, got, want), ...]"""
    idx = np.argwhere(got != want)[:limit]
    return [tuple(int(v) for v in i) + (int(got[tuple(i)]), int(want[tuple(i)])) for i in idx]
