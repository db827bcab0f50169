"""No GPU: the case table of tests/test_gpu_scan_blur.py is what it claims to be. (1) every partition edge of the two blur kernels is landed on
by at least one case; (2) the numpy restatement of the operation equals the oracle's co_gray_blur / co_scan_preprocess on every case, so the
reference the GPU test uses is held from a second side; (3) six wrong results a partitioning mistake would produce are all caught by comparing
the gray plane and the histogram, and three of them are NOT caught by the comparison the suite had before (binary image + threshold)."""
import numpy as np
import pytest

from tests import capture_formats as CF
from tests import scan_blur_cases as SB


def parts(cases, **kw):
    return [SB.partition(c.w, c.h, **kw) for c in cases]


STREAMING_EDGES = {
    "one group that is both first and last": lambda p: p["groups"] == 1,
    "3x3: last strip of 1 row": lambda p: p["unit"] == 3 and p["strips"] > 1 and p["last_strip_rows"] == 1,
    "one full block of 62 groups, exactly one strip": lambda p: p["block_groups"] == [62] and p["strips"] == 1 and p["last_strip_rows"] == 30,
    "blocks of 32 and 31": lambda p: p["block_groups"] == [32, 31],
    "a fifth strip of 1 row that opens a second workgroup": lambda p: p["strips"] == 5 and p["workgroups_y"] == 2 and p["last_strip_rows"] == 1,
    "blocks of 32 and 32": lambda p: p["block_groups"] == [32, 32],
    "3x3: last strip of 29 rows": lambda p: p["unit"] == 3 and p["last_strip_rows"] == 29,
    "3x3: blocks of 62 and 62, last strip of 2 rows": lambda p: p["unit"] == 3 and p["block_groups"] == [62, 62] and p["last_strip_rows"] == 2,
    "three blocks, the last one shorter": lambda p: p["block_groups"] == [42, 42, 41],
    "5x5: blocks of 47 and 47, whole strips": lambda p: p["unit"] == 5 and p["block_groups"] == [47, 47] and p["last_strip_rows"] == 30 and p["strips"] == 50,
    "5x5: last strip of 1 row, fewer than the radius": lambda p: p["unit"] == 5 and p["last_strip_rows"] == 1 < p["radius"],
    "5x5: blocks of 62 and 62, last strip of 2 rows": lambda p: p["unit"] == 5 and p["block_groups"] == [62, 62] and p["last_strip_rows"] == 2,
    "5x5: blocks of 48 and 47, last strip of 29 rows": lambda p: p["unit"] == 5 and p["block_groups"] == [48, 47] and p["last_strip_rows"] == 29,
}
TILED_EDGES = {
    "the smallest legal capture": lambda p: (p["w"], p["h"]) == (8, 8),
    "one tile plus one column, one tile plus one row": lambda p: (p["tiles_x"], p["last_tile_cols"], p["tiles_y"], p["last_tile_rows"]) == (2, 1, 2, 1),
    "one short tile; four tiles plus one row, a second workgroup": lambda p: p["tiles_x"] == 1 and p["last_tile_cols"] < 128 and p["tiles_y"] == 5
                                                                    and p["last_tile_rows"] == 1 and p["workgroups_y"] == 2,
    "last tile of 2 columns, byte stores": lambda p: p["last_tile_cols"] == 2 and p["stores"] == "byte",
    "last tile of 4 columns, dword stores": lambda p: p["last_tile_cols"] == 4 and p["stores"] == "dword",
    "5x5": lambda p: p["unit"] == 5,
    "9x9, last tile of 1 column": lambda p: p["unit"] == 9 and p["last_tile_cols"] == 1,
    "17x17": lambda p: p["unit"] == 17,
}


@pytest.mark.parametrize("edge", list(STREAMING_EDGES))
def test_a_case_lands_on_every_streaming_edge(edge):
    ps = parts(SB.STREAMING_3 + SB.STREAMING_5)
    assert all(p["kernel"] == "streaming" for p in ps)
    assert any(STREAMING_EDGES[edge](p) for p in ps), edge


@pytest.mark.parametrize("edge", list(TILED_EDGES))
def test_a_case_lands_on_every_tiled_edge(edge):
    ps = parts(SB.TILED)
    assert all(p["kernel"] == "tiled" for p in ps)
    assert any(TILED_EDGES[edge](p) for p in ps), edge


def test_the_other_groups_land_where_they_say():
    # blur unit: the sizes at which Scanner's rule changes kernel
    assert [SB.blur_unit(s, s) for s in (8, 499, 500, 1499, 1500, 2499, 2500, 4499, 4500)] == [3, 3, 3, 3, 5, 5, 9, 9, 17]
    # every format through both kernels, even heights for the 4:2:0 layouts
    for kernel in ("streaming", "tiled"):
        fmts = sorted(c.fmt for c in SB.FORMATS if SB.partition(c.w, c.h)["kernel"] == kernel)
        assert fmts == sorted(CF.FORMATS), kernel
    assert all(c.w % 2 == 0 and c.h % 2 == 0 for c in SB.FORMATS)
    # batches: tiled with frames that start off a 16-byte boundary, streaming with more than one frame
    kinds = {}
    for c in SB.BATCHES:
        p = SB.partition(c.w, c.h)
        kinds[p["kernel"]] = c
        assert c.n == 3
        if p["kernel"] == "tiled":
            assert p["frame_bytes_mod16"] != 0 and (2 * c.w * c.h * 3) % 16 != 0
    assert set(kinds) == {"streaming", "tiled"}
    # the misaligned capture: streaming where aligned, tiled where not -- the tiled RGB kernel on a width that is a multiple of 16
    c = SB.MISALIGNED
    assert c.fmt == 3 and c.w % 16 == 0
    assert SB.partition(c.w, c.h)["kernel"] == "streaming" and SB.partition(c.w, c.h, aligned=False)["kernel"] == "tiled"
    assert all(0 < off < 16 for off in SB.MISALIGNED_OFFSETS) and any(off % 4 for off in SB.MISALIGNED_OFFSETS) and any(off % 4 == 0 for off in SB.MISALIGNED_OFFSETS)
    assert sorted(SB.partition(SB.BY_NAME[k].w, SB.BY_NAME[k].h)["kernel"] for k in SB.PREPROCESS_TIE) == ["streaming", "tiled"]


@pytest.mark.parametrize("name", [c.name for c in SB.CASES])
def test_numpy_restatement_equals_the_oracle(name):
    case = SB.BY_NAME[name]
    buf, rgb = SB.capture(case)
    assert buf.shape == (case.n, CF.capture_bytes(case.w, case.h, case.fmt))
    _, gray, hist, thr = SB.reference(name)
    for k in range(case.n):
        plane, hs = SB.gray_blur(rgb[k])
        assert (plane == gray[k]).all(), (name, k, SB.differences(plane[None], gray[k][None]))
        assert (hs == hist[k]).all() and hs.sum() == case.w * case.h
        assert SB.otsu(hs, case.w, case.h) == thr[k]
    if case.n > 1:          # a batch whose frames were all alike could not show a histogram that leaked from one frame into the next
        assert len({hist[k].tobytes() for k in range(case.n)}) == case.n


def test_degenerate_histograms_are_what_they_are_meant_to_be():
    for level in (0, 100, 255):
        _, gray, hist, thr = SB.reference(f"flat{level}")
        assert hist[0][level] == 64 * 40 and thr[0] == 0        # one bin: q1 or q2 is below FLT_EPSILON at every step, nothing is ever chosen
    _, gray, hist, thr = SB.reference("halves")
    a, b = SB.HALVES_LEVELS
    assert hist[0][a] == hist[0][b] == 64 * 40 // 2 and thr[0] == a
    c = SB.BY_NAME["one-white-4000x2600"]
    _, gray, hist, thr = SB.reference(c.name)
    assert 1.0 / (c.w * c.h) < SB.FLT_EPSILON
    top = int(np.flatnonzero(hist[0])[-1])
    assert hist[0][top] == 1 and hist[0][0] > c.w * c.h - 200 and thr[0] == SB.ONE_WHITE_THRESHOLD < top


def binary_and_threshold_see(gray, hist, want_gray, want_thr, w, h):
    """what tests/test_gpu_extract.py compares: the threshold and the binarised image"""
    thr = SB.otsu(hist, w, h)
    return thr != want_thr or ((gray > thr) != (want_gray > want_thr)).any()


def test_planted_faults_are_caught_by_gray_and_histogram():
    case = SB.BY_NAME[SB.FAULT_CASE]
    p = SB.partition(case.w, case.h)
    assert p["kernel"] == "streaming" and p["nb"] > 1 and p["strips"] > 1
    _, rgb = SB.capture(case)
    _, gray, hist, thr = SB.reference(case.name)
    gray, hist, thr = gray[0], hist[0], int(thr[0])
    assert not binary_and_threshold_see(gray, hist, gray, thr, case.w, case.h)
    escaped = []
    for name, plant in SB.FAULTS.items():
        g, hs = plant(rgb[0], gray, hist)
        # the GPU test's three comparisons: plane against the oracle's, histogram against the oracle's, histogram against the plane's own
        caught = (g != gray).any() or (hs != hist).any() or (hs != np.bincount(g.reshape(-1), minlength=256)).any()
        assert caught, f"{name}: not caught on this case (a fault that changes nothing here needs another case)"
        if not binary_and_threshold_see(g, hs, gray, thr, case.w, case.h):
            escaped.append(name)
    print("faults the binary + threshold comparison misses on", case.name, ":", escaped)
    assert set(SB.MUST_ESCAPE_BINARY) <= set(escaped), escaped
