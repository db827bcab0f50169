"""Captures that are hard on the anchor search (Scanner::scan; libcimbar_amd/csrc/scan.hip.inc on the device): rotated and mirrored frames, decoy
bullseyes, patterns that fill the device kernels' fixed lists, unusual capture shapes, anchors at the capture's border, and quads at the
is_granular_scale boundary. CPU only (numpy + Pillow), seeded, deterministic. Every family returns (name, capture) pairs; captures are
(h, w, 3) uint8. tests/test_scan_hostile.py pins the oracle to the reference build on them, tests/test_gpu_scan_hostile.py the device to the
oracle."""
import ctypes
import math
import os
import re

import numpy as np

from tests import frames as F

W, H = 1280, 720


def _capacities():
    """the fixed capacities of the product build, read from libcimbar_amd/csrc/scan.hip.inc itself"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libcimbar_amd", "csrc", "scan.hip.inc")).read()
    text = re.sub(r"#ifdef CIMBAR_SCAN_TINY_LISTS.*?#else", "", text, flags=re.S)
    return {name: int(val) for name, val in re.findall(r"constexpr int (SCAN_[A-Z_]+) = (\d+);", text)}


_CAP = _capacities()
SCAN_ROW_PTS, SCAN_MAX_ROWS, SCAN_HMAX, SCAN_MAX_CAND = _CAP["SCAN_ROW_PTS"], _CAP["SCAN_MAX_ROWS"], _CAP["SCAN_HMAX"], _CAP["SCAN_MAX_CAND"]
SCAN_CONFIRM_POS, SCAN_ROW_POS, SCAN_CONF_MAX = _CAP["SCAN_CONFIRM_POS"], _CAP["SCAN_ROW_POS"], _CAP["SCAN_CONF_MAX"]
SCAN_LIST = 64          # no named constant in the source: the CAP = 64 of k_scan_confirm's LDS lists (s_col, s_diag, s_tmp; scan_vertical<KIND, 64> ...)

# co_scan_debug_counter selectors (oracle/cimbar_oracle_extract.c)
ROW_HITS, PRIMARY_HITS, CANDIDATES, EQUAL_SIZES, ROW_CHANGES, CONFIRM_CHANGES, CONFIRM_LIST, HIT_CONFIRMED, ROWS, OUTSIDE, BR_ROWS, BR_ROW_HITS, BR_HITS, \
    BR_CANDIDATES = range(14)


def measure(O, cam, frame_shape=(1024, 1024, 3)):
    """the oracle library O on one capture: anchors found, their rectangles, the counters of the search, Extractor::extract's status, corners and
    frame. What the GPU tests compare the device with, and what the CPU tests compare with the reference build."""
    def P(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    h, w = cam.shape[:2]
    binimg = np.zeros((h, w), np.uint8)
    a = np.zeros(16, np.int32)
    O.co_scan_preprocess(P(cam), w, h, P(binimg))
    n = O.co_scan_anchors(P(binimg), w, h, P(a))
    cnt = [O.co_scan_debug_counter(k) for k in range(14)]
    out = np.zeros(frame_shape, np.uint8)
    c8 = (ctypes.c_float * 8)()
    st = O.co_extract(P(cam), w, h, P(out), c8)
    return dict(found=n, anchors=a[:4 * min(n, 4)].reshape(-1, 4).copy(), cnt=cnt, status=st, corners=list(c8), frame=out)


def measure_families(synth, O):
    """every mode-B family once: name -> [(case name, capture, measure())]"""
    return {fam: [(name, cam, measure(O, cam)) for name, cam in gen(synth)] for fam, gen in FAMILIES.items()}


def clean(synth, n=4, seed=9):
    return F.clean_frames(synth, n, seed=seed)[1]


def rotated_quad(cx, cy, half_w, half_h, deg, mirror=None):
    """the quad (tl, tr, bl, br) of a frame centred on (cx, cy) and turned by deg (clockwise on the screen); mirror 'h' / 'v' swaps its sides"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    pts = [(-half_w, -half_h), (half_w, -half_h), (-half_w, half_h), (half_w, half_h)]
    if mirror == "h":
        pts = [pts[1], pts[0], pts[3], pts[2]]
    elif mirror == "v":
        pts = [pts[2], pts[3], pts[0], pts[1]]
    return tuple((int(round(cx + x * c - y * s)), int(round(cy + x * s + y * c))) for x, y in pts)


def bullseye(img, cx, cy, side, kind=114, value=255):
    """a hand-drawn anchor of `side` pixels centred on (cx, cy): bright : dark : bright : dark : bright = 1:1:4:1:1 (kind 114, the three large anchors)
    or 1:2:2:2:1 (kind 122, the small bottom-right one) along every line through its centre"""
    ring, core = (side / 8.0, side / 4.0) if kind == 114 else (side / 8.0, 3 * side / 8.0)

    def box(inset, v):
        x0, y0 = int(round(cx - side / 2.0 + inset)), int(round(cy - side / 2.0 + inset))
        x1, y1 = int(round(cx + side / 2.0 - inset)), int(round(cy + side / 2.0 - inset))
        img[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = v
    box(0, value)
    box(ring, 0)
    box(core, value)


def with_frame(synth, quad, w=W, h=H, background=0, k=0, blur=0.0):
    return np.ascontiguousarray(F.camera_frame(clean(synth)[k % 4], width=w, height=h, quad=quad, background=background, blur=blur))


# ---------------------------------------------------------------------------------------------------------------------------- orientation
ORIENTATION_ANGLES = [0, 4, -4, 8, -8, 11, -11, 87, 90, 93, 177, 180, 183, 267, 270, 273, 20, 45]


def orientation(synth):
    """sort_top_to_bottom's geometry: the frame upright, tilted, on its side, upside down, mirrored; 20 and 45 degrees are beyond what the row scans
    find (they must fail the same way everywhere)"""
    out = []
    for k, deg in enumerate(ORIENTATION_ANGLES):
        out.append(("rot%+d" % deg, with_frame(synth, rotated_quad(636, 354, 290, 290, deg), background=(0, 40, 16)[k % 3], k=k)))
    out.append(("mirror-h", with_frame(synth, rotated_quad(636, 354, 290, 290, 2, "h"), k=1)))
    out.append(("mirror-v", with_frame(synth, rotated_quad(636, 354, 290, 290, -2, "v"), k=2)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- decoys
DECOY_QUAD = ((52, 62), (632, 64), (50, 642), (630, 644))          # anchors of 34 px in the quad's corners; the bottom-right one's centre near (612, 626)


def decoys_base(synth):
    """the decoy-free capture every `decoys` case starts from"""
    return with_frame(synth, DECOY_QUAD)


def decoys(synth):
    """hand-drawn bullseyes beside (and on) a good frame. displace-*: a 1:1:4:1:1 bullseye larger than / as large as the real anchors enters the top
    three; window-*: something inside the bottom-right search window (a 1:2:2:2:1 bullseye in front of the real fourth anchor, or the fourth anchor
    painted over: the search finds nothing); filtered-*: bullseyes well under filter_candidates' size cutoff"""
    base = decoys_base(synth)
    out = []

    def case(name, fn):
        img = base.copy()
        fn(img)
        out.append((name, img))
    case("displace-larger", lambda im: bullseye(im, 1000, 360, 64))
    case("displace-larger-top", lambda im: bullseye(im, 900, 60, 48))
    case("displace-equal", lambda im: bullseye(im, 1000, 600, 32))
    case("displace-five", lambda im: [bullseye(im, x, y, s) for x, y, s in ((800, 120, 56), (1000, 240, 48), (1150, 400, 40), (850, 480, 64), (1100, 620, 44))])
    case("window-decoy-122", lambda im: bullseye(im, 656, 596, 36, kind=122))
    case("window-blank", lambda im: im.__setitem__((slice(604, 650), slice(590, 636)), 0))
    case("window-decoy-114", lambda im: bullseye(im, 656, 600, 30))
    case("filtered-one", lambda im: bullseye(im, 1000, 360, 16))
    case("filtered-many", lambda im: [bullseye(im, 780 + 60 * (k % 8), 96 + 120 * (k // 8), 16 + 2 * (k % 3)) for k in range(12)])
    case("filtered-and-larger", lambda im: [bullseye(im, 1000, 360, 16), bullseye(im, 1000, 600, 60)])
    return out


# ---------------------------------------------------------------------------------------------------------------------------- pressure
PRESSURE_QUAD = ((12, 62), (592, 64), (10, 642), (590, 644))       # a 580 px frame at the left, below scan row 48; scan rows are 12 px apart at 1280x720


def comb(img, x0, y0, y1, repeats, period=34):
    """`repeats` groups of vertical bars 3:5:14:5:3 (+ a 4 px gap) from x0 on, in rows [y0, y1): every scan row through them yields one hit per group.
    The widths pass the 1:1:4:1:1 test as drawn and with every bright run a pixel wider on both sides, which is what a low Otsu threshold (a capture
    that also holds a frame) makes of them after the blur"""
    for r in range(repeats):
        x = x0 + r * period
        img[y0:y1, x:x + 3] = 255
        img[y0:y1, x + 8:x + 22] = 255
        img[y0:y1, x + 27:x + 30] = 255


ROW_W = 3072                                                        # so that 72 comb groups and a frame fit side by side
ROW_QUAD = tuple((x + 2470, y) for x, y in PRESSURE_QUAD)          # the frame at the right; its top anchors cross scan rows 72 and 84
ROW_FRAME_HITS = 2                                                  # hits of the frame itself on scan row 72: its two top anchors


def row_comb(synth, hits):
    """scan row y = 72 holds `hits` hits: a comb, and to its RIGHT the frame's two top anchors, so that the anchors' hits are the last of the row's
    list (SCAN_ROW_PTS) -- a list that dropped or overwrote its last entries would lose an anchor"""
    img = with_frame(synth, ROW_QUAD, w=ROW_W)
    comb(img, 8, 68, 77, hits - ROW_FRAME_HITS)
    return img


def total_comb(synth, total, frame):
    """`total` hits spread over rows of at most 40 (under SCAN_ROW_PTS): the per-capture hit list (SCAN_HMAX). With a frame the comb stands to
    its right, 36 groups to a row, and the frame's own hits come on top (FRAME_HITS: they depend a little on the Otsu threshold, so on the comb).
    1920x720"""
    img = with_frame(synth, PRESSURE_QUAD, w=1920) if frame else np.zeros((H, 1920, 3), np.uint8)
    x0 = 624 if frame else 8
    per = 36 if frame else 40
    y = 12
    left = total - (FRAME_HITS[total] if frame else 0)
    while left > 0:
        n = min(per, left)
        comb(img, x0, y - 3, y + 4, n)          # 7 px tall around scan row y: that row alone
        left -= n
        y += 12
    assert y <= H, "comb does not fit"
    return img


# primary hits of PRESSURE_QUAD's frame next to the comb of each total (measured on the oracle; tests/test_scan_hostile.py asserts the totals)
FRAME_HITS = {512: 130, 1023: 19, 1024: 19, 1025: 19, 1536: 10}
FRAME_CANDIDATES = 3


def field(synth, count, frame):
    """`count` candidates before filter_candidates (SCAN_MAX_CAND; 16, where std::sort stops being an insertion sort). Without a frame: bullseyes of
    `count` different sizes from 26 px up. With one: small bullseyes (20 px, under the cutoff the frame's anchors set) beside it, so that the answer
    is the frame's quad; those repeat sizes"""
    if frame:
        img = with_frame(synth, PRESSURE_QUAD)
        n = count - FRAME_CANDIDATES
        cols = 13
        for k in range(n):
            bullseye(img, 640 + 48 * (k % cols), 36 + 60 * (k // cols), 20)
        assert n <= cols * 11
        return img
    w, h, skip = (W, H, 12) if count <= 18 else (2560, 1440, 24)          # the larger fields need a larger capture
    img = np.zeros((h, w, 3), np.uint8)
    sizes = [2 * skip + 2 + 2 * k for k in range(count)]          # 2 px apart: the measured extents wobble by one, the sizes stay distinct
    x, y, rowh = 10, 0, 0
    placed = []

    def clash(cx, cy, s):
        # no bullseye's centre column may run through the bright core of one above or below it: the column scan of a hit reaches 1.5 sizes up and
        # down, would confirm that one too, off-centre, and the two candidates it then gets would have equal sizes by accident
        return any(abs(cx - px) < max(s, ps) // 4 + 4 and abs(cy - py) < 3 * max(s, ps) // 2 + skip for px, py, ps in placed)
    for s in sizes:          # shelves: left to right, a new shelf when the row is full; centres on scan rows (multiples of skip)
        pitch = ((s + 16 + skip - 1) // skip) * skip
        while True:
            cy = (y + pitch // 2 + skip - 1) // skip * skip
            while x + s + 10 <= w and clash(x + s // 2, cy, s):
                x += 4
            if x + s + 10 <= w:
                break
            x, y, rowh = 10, y + rowh, 0
        placed.append((x + s // 2, cy, s))
        bullseye(img, x + s // 2, cy, s)
        x += s + w // 30 + 4          # centres more than w / 30 apart: never merged
        rowh = max(rowh, pitch + skip)
    assert y + rowh <= h, "field does not fit"
    return img


def confirm_comb(stripes, w, h, anchors=0):
    """a 1:1:4:1:1 pattern of very wide bars, cut into `stripes` horizontal stripes 2 px on / 2 px off: the column scan of a row hit runs 3 hit-widths
    up and down and crosses 2 * stripes run boundaries (SCAN_CONFIRM_POS). anchors: rows added below for four hand-drawn anchors, so that the answer
    is a quad (their own column scans are short and the comb's run between them)"""
    u = (w - 40) // 8
    xs = np.zeros(w, bool)
    x0 = (w - 8 * u) // 2
    xs[x0:x0 + u] = xs[x0 + 2 * u:x0 + 6 * u] = xs[x0 + 7 * u:x0 + 8 * u] = True
    ys = np.zeros(h, bool)
    y0 = max(8, (h - 4 * stripes) // 2) // 4 * 4
    for k in range(stripes):
        ys[y0 + 4 * k:y0 + 4 * k + 2] = True
    assert y0 + 4 * stripes <= h
    img = (ys[:, None] & xs[None, :]).astype(np.uint8) * 255
    img = np.ascontiguousarray(np.repeat(img[:, :, None], 3, 2))
    if anchors:
        low = drawn_anchors(w, anchors, 200, 120, w - 200, anchors - 120, 100)
        img = np.ascontiguousarray(np.concatenate([img, low], 0))
    return img


def pressure(synth):
    """each capacity swept: at half or less, within +-2, at 1.5x or more. name = <list>-<target>[+frame]"""
    out = []
    for n in (22, 46, 47, 48, 49, 50, 72):
        out.append(("row-%d+frame" % n, row_comb(synth, n)))
    for n, fr in ((512, True), (1022, False), (1023, True), (1024, True), (1025, True), (1026, False), (1536, True)):
        out.append(("total-%d%s" % (n, "+frame" if fr else ""), total_comb(synth, n, fr)))
    for n, fr in ((8, True), (14, False), (15, True), (16, False), (17, False), (18, False), (32, False), (62, False), (63, False), (64, True), (65, False),
                  (66, False), (96, True)):
        out.append(("cand-%d%s" % (n, "+frame" if fr else ""), field(synth, n, fr)))
    out.append(("confirm-512", confirm_comb(256, 1400, 1400)))
    out.append(("confirm-1022", confirm_comb(511, 1400, 2200)))
    out.append(("confirm-1024+anchors", confirm_comb(512, 1400, 2200, anchors=600)))
    out.append(("confirm-1026", confirm_comb(513, 1400, 2200)))
    out.append(("confirm-1600", confirm_comb(800, 1400, 3400)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- shapes
def drawn_anchors(w, h, x0, y0, x1, y1, side):
    """a capture that holds nothing but four hand-drawn anchors: three 1:1:4:1:1 ones and the smaller 1:2:2:2:1 one at the bottom right"""
    img = np.zeros((h, w, 3), np.uint8)
    bullseye(img, x0, y0, side)
    bullseye(img, x1, y0, side)
    bullseye(img, x0, y1, side)
    bullseye(img, x1, y1, side * 3 // 4, kind=122)
    return img


def shapes(synth):
    """tall narrow captures (more than SCAN_MAX_ROWS scan rows), a wide flat one, and the smallest the reference handles (256x144: skip = 2). The
    first case of every shape is one the search locks onto (frame sizes and contents found by trying; at 256x144 no drawn FRAME locks, its cells are
    a pixel wide, so that one holds hand-drawn anchors); the others fail, the same way everywhere"""
    out = []
    for (w, h, quad, k) in ((480, 1280, rotated_quad(240, 640, 238, 238, 0), 1), (480, 1280, rotated_quad(240, 640, 215, 215, 2), 0),
                            (540, 1920, rotated_quad(270, 1200, 259, 259, 0), 1), (540, 1920, rotated_quad(270, 500, 264, 264, 2), 2),
                            (1920, 540, rotated_quad(1300, 270, 248, 248, 0), 1), (1920, 540, rotated_quad(1300, 270, 259, 259, 0), 3)):
        out.append(("%dx%d-%d" % (w, h, len(out)), with_frame(synth, quad, w=w, h=h, k=k)))
    out.append(("256x144-6", drawn_anchors(256, 144, 70, 22, 180, 122, 24)))
    out.append(("256x144-7", with_frame(synth, rotated_quad(128, 72, 68, 68, 0), w=256, h=144)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- edges
ANCHOR_INSET = 0          # the anchors' outer rings start at the quad's corners


def edges(synth):
    """a 580 px frame pushed against the capture's left / top / right / bottom border: the nearest anchors' outer ring `d` px inside it (3, 2, 1),
    touching it (0) or cut by it (-3, -12), and quads partly out of view. inside = the confirm scans stay in the image (decided by the oracle's
    counter in the tests, not here)"""
    out = []
    side = 580
    for d in (3, 2, 1, 0, -3, -12):
        off = d - ANCHOR_INSET
        out.append(("left%+d" % d, with_frame(synth, ((off, 50), (off + side, 50), (off, 50 + side), (off + side, 50 + side)), k=len(out))))
        out.append(("top%+d" % d, with_frame(synth, ((300, off), (300 + side, off), (300, off + side), (300 + side, off + side)), k=len(out))))
    for d in (2, 0, -3):
        off = d - ANCHOR_INSET
        out.append(("right%+d" % d, with_frame(synth, ((W - off - side, 50), (W - off, 50), (W - off - side, 50 + side), (W - off, 50 + side)), k=len(out))))
        out.append(("bottom%+d" % d, with_frame(synth, ((300, H - off - side), (300 + side, H - off - side), (300, H - off), (300 + side, H - off)), k=len(out))))
    out.append(("half-out-left", with_frame(synth, ((-300, 62), (280, 62), (-300, 642), (280, 642)), k=1)))
    out.append(("corner-out", with_frame(synth, ((700, 200), (1320, 190), (710, 820), (1330, 810)), k=2)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- scale
SCALE_CAPTURE = {68: (2560, 1440), 67: (1920, 1080), 66: (1920, 1080)}
# half steps: the measured centres are whole pixels. The last eight put ONE axis at the boundary and the other clearly above it
SCALE_STEPS = [(d / 2.0, d / 2.0) for d in range(-5, 6)] + [(2, -2), (-2, 2), (0, 2), (0.5, 2), (-0.5, 2), (1, 2.5), (2, 0), (2, 0.5), (2, -0.5), (2.5, 1)]


def scale(synth_mode, mode):
    """near-square upright quads whose anchor-centre distances are IMG_W + dx and IMG_H + dy: is_granular_scale's `>` (status 1 above, 2 at or below).
    synth_mode: a FrameSynth of `mode`. The anchors' centres sit 30 frame pixels inside the frame's corners (Deskewer.h:28-32)."""
    geo = synth_mode.geo
    w, h = SCALE_CAPTURE[mode]
    fr = F.clean_frames(synth_mode, 1, seed=21)[1][0]
    out = []
    for dx, dy in SCALE_STEPS:
        qw = (geo.IMG_W + dx) * geo.IMG_W / (geo.IMG_W - 60.0)
        qh = (geo.IMG_H + dy) * geo.IMG_H / (geo.IMG_H - 60.0)
        x0, y0 = (w - geo.IMG_W) // 2 - 32, (h - geo.IMG_H) // 2 - 32          # the top-left corner stays put: the distances move in steps of one
        quad = tuple((int(round(x)), int(round(y))) for x, y in ((x0, y0), (x0 + qw, y0), (x0, y0 + qh), (x0 + qw, y0 + qh)))
        out.append(("scale%d%+.1f%+.1f" % (mode, dx, dy), np.ascontiguousarray(F.camera_frame(fr, width=w, height=h, quad=quad, background=0))))
    return out


FAMILIES = {"orientation": orientation, "decoys": decoys, "pressure": pressure, "shapes": shapes, "edges": edges}
