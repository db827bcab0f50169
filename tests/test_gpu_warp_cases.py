"""GPU: the deskew warp (k_warp_matrices' matrix, k_warp / remap_bilinear / capture_pair, and for 4:2:0 captures k_roi_boxes -> k_convert_roi ->
k_warp<3>) against the oracle's co_deskew, bit-exact, on the cases of tests/warp_cases.py: hostile quads (mirrored, rotated, self-intersecting,
singular, fractional, huge, non-finite), capture widths that are no multiple of 8, captures down to 2x2, every capture format, every mode's frame
size. The oracle is pinned to the reference build on the same cases in tests/test_warp_cases.py, where the table's coverage conditions live."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from tests import warp_cases as WC
from tests.test_gpu_flood_verify import decoder_with

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = WC.table()
GUARD = 4096


def corners_of(cases):
    return np.stack([c.corners for c in cases])


def differing(got, want, cases):
    return [f"{c.name}: {int((got[k] != want[k]).sum())} bytes differ" for k, c in enumerate(cases) if not (got[k] == want[k]).all()]


def assert_frames(got, want, cases, what):
    bad = differing(got, want, cases)
    assert not bad, f"{what}: " + "; ".join(bad)


def assert_batches(run, batches, what):
    """run(cases) -> frames for every batch, then one verdict that names every case that differs"""
    bad = [b for cases, want in batches for b in differing(run(cases), want, cases)]
    assert not bad, f"{what}: {len(bad)} cases differ; " + "; ".join(bad)


def deskew(dec, cases, caps=None):
    c = cases[0]
    return dec.deskew_batch(WC.batch_captures(cases) if caps is None else caps, corners_of(cases), size=(c.w, c.h), fmt=c.fmt)


def deskew_device(dec, cases):
    """the same call with device pointers on the caller's stream; the frames sit between two guard patterns, which must survive"""
    c = cases[0]
    n, per = len(cases), dec.geo.FRAME_RGB_BYTES
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(WC.batch_captures(cases)).to(dev)
    d_out = torch.full((GUARD + n * per + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    dec.deskew_batch_device(d_in.data_ptr(), c.w, c.h, n, corners_of(cases), d_out.data_ptr() + GUARD, st, fmt=c.fmt)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n * per:] == 0xA5).all(), f"{c.w}x{c.h} format {c.fmt}: guard bytes around the frames were written"
    return out[GUARD:GUARD + n * per].reshape(n, *dec.geo.FRAME_SHAPE)


@pytest.fixture(scope="module", params=WC.FORMATS)
def fmt_batches(request):
    """the table's cases of one format, one batch per capture size, with the oracle's frames (computed once per format)"""
    return [(cases, WC.expected(cases)) for cases in WC.batches([c for c in TABLE if c.fmt == request.param]).values()]


@pytest.fixture(scope="module", params=[67, 66])
def mode_batches(request):
    mode = request.param
    dec = D.HipDecoder(0, mode)
    yield mode, dec, [(cases, WC.expected(cases)) for cases in WC.batches(WC.mode_table(mode)).values()]
    dec.close()


def test_deskew_batch_matches_oracle(hip_decoder, fmt_batches):
    """every case of the table, all cases of one capture size and format in one call with per-capture quads. 4:2:0 captures take the default two-pass
    route here: k_convert_roi's general path for every width that is no multiple of 8"""
    assert_batches(lambda cases: deskew(hip_decoder, cases), fmt_batches, "deskew_batch")


def test_direct_warp_kernels_match_oracle(fmt_batches):
    """CIMBAR_HIP_WARP_TWOPASS=0: k_warp<12> / k_warp<420> with their per-tap chroma pairs on the same quads and widths (RGB and RGBA captures go
    through their own kernels either way: the same frames from a second context)"""
    d = decoder_with({"CIMBAR_HIP_WARP_TWOPASS": "0"})
    try:
        assert_batches(lambda cases: deskew(d, cases), fmt_batches, "deskew_batch, conversion inside the warp kernel")
    finally:
        d.close()


def test_deskew_batch_device_matches_oracle_and_stays_inside_its_output(hip_decoder, fmt_batches):
    assert_batches(lambda cases: deskew_device(hip_decoder, cases), fmt_batches, "deskew_batch with device pointers")


def test_launch_order_gives_the_same_bytes(tmp_path):
    """CIMBAR_HIP_WARP_ORDER=0 (tiles in launch order, not dealt to the XCDs in runs) is read once per process: one batch in a child process"""
    cases = [c for c in TABLE if (c.w, c.h, c.fmt) == (*WC.ODD8, 12)]
    out = str(tmp_path / "frames.npy")
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from libcimbar_amd import HipDecoder; from tests import warp_cases as WC; "
            "cases = [c for c in WC.table() if (c.w, c.h, c.fmt) == (*WC.ODD8, 12)]; d = HipDecoder(0); "
            "np.save(%r, d.deskew_batch(WC.batch_captures(cases), np.stack([c.corners for c in cases]), size=WC.ODD8, fmt=12)); d.close(); print('ok')") % (ROOT, out)
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CIMBAR_HIP_WARP_ORDER="0"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    assert_frames(np.load(out), WC.expected(cases), cases, "deskew_batch in launch order")


def test_other_frame_sizes_match_oracle(mode_batches):
    """modes 67 (1024x720) and 66 (736x637: the last 64-column tile is half empty): inscribed, overhanging, mirrored, bow-tie and singular quads in
    every format at 1920x1080 and 1282x978 against the oracle built for the mode -- host and device entry points, and for 4:2:0 both routes"""
    mode, dec, batches = mode_batches
    direct = decoder_with({"CIMBAR_HIP_WARP_TWOPASS": "0"}, mode)
    try:
        assert all(want.shape[1:] == dec.geo.FRAME_SHAPE for _, want in batches)
        assert_batches(lambda cases: deskew(dec, cases), batches, f"mode {mode} deskew_batch")
        assert_batches(lambda cases: deskew_device(dec, cases), batches, f"mode {mode} deskew_batch with device pointers")
        assert_batches(lambda cases: deskew(direct, cases), [b for b in batches if b[0][0].fmt in (12, 420)], f"mode {mode} deskew_batch, conversion inside the warp kernel")
    finally:
        direct.close()


@pytest.mark.parametrize("mode", [4, 8])
def test_modes_of_the_same_frame_size(mode):
    cases = WC.mode_table(mode)
    d = D.HipDecoder(0, mode)
    try:
        assert_frames(deskew(d, cases), WC.expected(cases), cases, f"mode {mode} deskew_batch")
    finally:
        d.close()


PAIR_QUADS = ("inscribed", "overhang", "mirrored", "bowtie", "far", "rot90", "perspective", "fractional")


def round_robin(w, h, fmt, n, mode):
    """n captures of w x h: eight distinct (capture, quad) pairs dealt round robin, and the oracle's frame of each pair"""
    pairs = [WC.make(q, w, h, fmt, mode) for q in PAIR_QUADS]
    caps, want = WC.batch_captures(pairs), WC.expected(pairs)
    idx = np.arange(n) % len(pairs)
    return pairs, np.ascontiguousarray(caps[idx]), np.ascontiguousarray(corners_of(pairs)[idx]), want, idx


def assert_round_robin(got, want, pairs, idx, what):
    bad = [f"capture {k} ({pairs[j].name}): {int((got[k] != want[j]).sum())} bytes differ" for k, j in enumerate(idx) if not (got[k] == want[j]).all()]
    assert not bad, f"{what}: {len(bad)} of {len(idx)} differ; " + "; ".join(bad[:6])


@pytest.mark.parametrize("fmt", [12, 420])
def test_two_pass_route_across_its_pass_boundary(fmt):
    """more 4:2:0 captures in one call than a pass of the two-pass route holds (WARP_CHUNK = 512): 520 of 96x64, the second pass short. In mode 66,
    whose frames are the smallest (the pass logic does not know the mode)"""
    d = D.HipDecoder(0, 66)
    try:
        pairs, caps, corners, want, idx = round_robin(96, 64, fmt, 520, 66)
        got = d.deskew_batch(caps, corners, size=(96, 64), fmt=fmt)
        assert_round_robin(got, want, pairs, idx, "520 captures in one call")
    finally:
        d.close()


@pytest.mark.parametrize("fmt", [12, 420])
def test_two_pass_route_with_a_handful_of_captures_per_pass(fmt):
    """CIMBAR_HIP_WARP_SCRATCH_MB=1: a converted 322x242 capture is 233 772 bytes, so a pass holds four; eleven captures go 4 + 4 + 3"""
    assert (1 << 20) // (322 * 242 * 3) == 4
    d = decoder_with({"CIMBAR_HIP_WARP_SCRATCH_MB": "1"}, 66)
    try:
        pairs, caps, corners, want, idx = round_robin(322, 242, fmt, 11, 66)
        got = d.deskew_batch(caps, corners, size=(322, 242), fmt=fmt)
        assert_round_robin(got, want, pairs, idx, "eleven captures, four per pass")
    finally:
        d.close()


@pytest.mark.parametrize("fmt", [12, 420])
def test_nothing_outside_a_captures_own_box_is_read(fmt):
    """one context: a batch whose boxes are the whole capture leaves its conversion in the scratch; the next batch -- same size and count, other
    content, boxes of a few dozen pixels -- must come out as the oracle's, i.e. without a byte of what the first left behind"""
    w, h = WC.ODD8
    big = [WC.make("overhang", w, h, fmt)] * 4
    small = [WC.Case(f"small-box-{k}", w, h, fmt, "small", np.array([x, y, x + 40, y + 2, x - 2, y + 30, x + 42, y + 31], np.float32), 68)
             for k, (x, y) in enumerate(((600, 400), (10, 12), (1225, 930), (700, 5)))]
    caps_small = np.ascontiguousarray(WC.batch_captures(small)[:, ::-1])          # (not the bytes the first batch had at the same place)
    d = D.HipDecoder(0)
    try:
        assert_frames(deskew(d, big), WC.expected(big), big, "whole-capture boxes")
        O = WC.pyref.oracle_lib()
        want = np.stack([WC.oracle_frame(O, WC.rgb_view(O, caps_small[k], w, h, fmt), c.corners) for k, c in enumerate(small)])
        assert_frames(deskew(d, small, caps_small), want, small, "small boxes after whole-capture boxes")
    finally:
        d.close()


def test_malformed_calls_are_refused_and_the_context_goes_on(hip_decoder):
    lib = D.load_library()
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(hip_decoder.geo.FRAME_RGB_BYTES, np.uint8)
    corners = np.array([10, 10, 50, 10, 10, 50, 50, 50], np.float32)

    def call(w, h, fmt):
        return lib.cimbar_hip_deskew_batch_fmt(hip_decoder._ctx, buf.ctypes.data, w, h, fmt, 1, D.MEM_HOST, corners.ctypes.data, out.ctypes.data, D.MEM_HOST, None)
    for fmt in WC.FORMATS:
        for (w, h) in ((1, 64), (64, 1), (0, 0), (1, 1)):
            assert call(w, h, fmt) == -1, (w, h, fmt)              # EINVAL
    for fmt in (12, 420):
        for (w, h) in ((63, 64), (64, 63), (3, 3)):
            assert call(w, h, fmt) == -2, (w, h, fmt)              # EDIM
    cases = [c for c in TABLE if (c.w, c.h, c.fmt) == (10, 6, 420)]
    assert_frames(deskew(hip_decoder, cases), WC.expected(cases), cases, "deskew_batch after refused calls")
