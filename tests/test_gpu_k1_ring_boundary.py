"""The threshold kernel where a strip's walk ends. A wavefront walks its strip in passes over a ring of RING = 2 RAD + 2 rows (6 without the
sharpen pass, 8 with it): full passes in a loop, then the last total % RING steps once, where total = the strip's rows + 2 RAD. A mistake in
that hand-over (a step too few or too many, a row taken from the wrong prefetch buffer, a ring slot out of phase) shows in the last rows of a
strip or in the first rows of the next -- so the bit plane is held against the oracle on the first strip, a middle strip and the last strip,
which end their walk at different total % RING, and then on every other row; and the kernel's second product, the undrifted cell means, against
a numpy restatement of Cell.h.

The strips, by image rows [y_begin, y_end), and `total % 6` without / `total % 8` with the sharpen pass (strips start on cell rows: y = OFFSET + 9 *
cell row; the first strip begins at row 0 and the last one ends with the image):

  mode        short strips (cell rows)   first        middle             last            tall strips   first        middle            last
  68 / 4 / 8  56 of 2                    [0, 26) 0 0  [512, 530) 4 0     [998, 1024) 0 0  16 of 7      [0, 71) 3 5  [512, 575) 1 5    [953, 1024) 3 5
  67          39 of 2                    [0, 27) 1 1  [351, 369) 4 0     [693, 720) 1 1   16 of 5      [0, 54) 4 4  [369, 414) 1 3    [684, 720) 4 2
  66          23 of 3                    [0, 36) 4 2  [306, 333) 1 1     [603, 637) 2 0   12 of 6      [0, 63) 1 5  [333, 387) 4 4    [603, 637) 2 0

(mode 67's and 66's last tall strips are shorter than the others: three cell rows where the others hold five and six).

The batch is three frames: uniform noise (every residue of the division by 36, every carry of the column sums), all 0 and all 255 (the column
sums at their two ends)."""
import numpy as np
import pytest

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from oracle import pyref
from oracle.pyref import P
from tests.test_gpu_flood_verify import decoder_with

pytestmark = pytest.mark.gpu

MODES = [68, 67, 66, 4, 8]
CELL_ROWS = {"short": {68: 2, 67: 2, 66: 3, 4: 2, 8: 2}, "tall": {68: 7, 67: 5, 66: 6, 4: 7, 8: 7}}   # K1_CELLROWS / K1_TALLROWS of mode.hip.inc


def strips_of(geo, rows):
    """[(y_begin, y_end)] of the kernel's strips of `rows` cell rows"""
    n = (geo.DIM_Y + rows - 1) // rows
    return [(0 if s == 0 else geo.OFFSET + s * rows * geo.PITCH, geo.IMG_H if s == n - 1 else geo.OFFSET + (s + 1) * rows * geo.PITCH) for s in range(n)]


_frames, _planes = {}, {}


def frames_of(mode):
    """noise, all 0, all 255: one batch per geometry (the legacy modes 4 and 8 have mode 68's, and share its frames and its oracle planes)"""
    geo = geometry.for_mode(mode)
    key = (geo.IMG_W, geo.IMG_H)
    if key not in _frames:
        fr = np.empty((3, geo.IMG_H, geo.IMG_W, 3), np.uint8)
        fr[0] = np.random.default_rng(6100 + geo.IMG_H).integers(0, 256, fr[0].shape, dtype=np.uint8)
        fr[1] = 0
        fr[2] = 255
        _frames[key] = fr
    return _frames[key]


def oracle_planes(mode, pre):
    """co_threshold_bitplane of the three frames, as rows of IMG_W / 8 bytes: computed once per (geometry, pre) and shared"""
    geo = geometry.for_mode(mode)
    key = (geo.IMG_W, geo.IMG_H, int(pre))
    if key not in _planes:
        O = pyref.oracle_lib(mode)
        out = []
        for f in frames_of(mode):
            want = np.zeros(geo.IMG_W * geo.IMG_H // 8, np.uint8)
            O.co_threshold_bitplane(P(np.ascontiguousarray(f)), geo.IMG_W, geo.IMG_H, int(pre), P(want))
            out.append(want.reshape(geo.IMG_H, geo.IMG_W // 8))
        _planes[key] = np.stack(out)
    return _planes[key]


def cell_means(frames, geo):
    """Cell.h:30-62 mean_rgb of the inner 6x6 of every cell at its grid position: uint16 channel sums, divided by 36 with the remainder dropped"""
    h, w = geo.DIM_Y * geo.PITCH, geo.DIM_X * geo.PITCH
    cells = frames[:, geo.OFFSET:geo.OFFSET + h, geo.OFFSET:geo.OFFSET + w].reshape(len(frames), geo.DIM_Y, geo.PITCH, geo.DIM_X, geo.PITCH, 3)
    sums = cells[:, :, 1:7, :, 1:7].astype(np.uint32).sum(axis=(2, 4))
    assert sums.max() <= 36 * 255
    m = sums // 36
    return m[..., 0] | (m[..., 1] << 8) | (m[..., 2] << 16)


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("which", ["short", "tall"])
@pytest.mark.parametrize("mode", MODES)
def test_strip_ends_and_cell_means(mode, which, pre):
    geo = geometry.for_mode(mode)
    frames = frames_of(mode)
    want = oracle_planes(mode, pre)
    dec = decoder_with({"CIMBAR_HIP_K1_STRIPS": which}, mode)
    try:
        dec.decode_batch(frames, should_preprocess=pre)
        got = dec.tap(D.TAP_BITPLANE, 3).reshape(want.shape)
        means = dec.tap(D.TAP_CELL_MEANS, 3)
    finally:
        dec.close()
    strips = strips_of(geo, CELL_ROWS[which][mode])
    ring = 8 if pre else 6
    for s in (0, len(strips) // 2, len(strips) - 1):
        y0, y1 = strips[s]
        bad = np.argwhere(got[:, y0:y1] != want[:, y0:y1])
        assert bad.size == 0, (f"strip {s} = rows [{y0}, {y1}), total % RING = {(y1 - y0 + ring - 2) % ring}: {len(bad)} bit plane bytes differ, "
                               f"first in frame {bad[0][0]} row {y0 + bad[0][1]} byte {bad[0][2]}")
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bit plane bytes differ, first in frame {bad[0][0]} row {bad[0][1]} byte {bad[0][2]}"
    want_means = cell_means(frames, geo)
    assert (want_means[1] == 0).all() and (want_means[2] == 0xFFFFFF).all()
    bad = np.argwhere(means != want_means)
    assert bad.size == 0, (f"{len(bad)} cell means differ, first in frame {bad[0][0]} cell row {bad[0][1]} column {bad[0][2]}: "
                           f"{means[tuple(bad[0])]:#08x} for {want_means[tuple(bad[0])]:#08x}")
