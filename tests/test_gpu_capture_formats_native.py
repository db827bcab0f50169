"""GPU: the capture formats of native receivers -- NV21 (21), YUYV (422), UYVY (4221), BGR (30), BGRA (40), include/cimbar_hip.h -- through every
kernel that reads a capture (X1 gray + blur, X4 warp, the convert-ahead pass, undistort) and every front end that takes `format`. Everything is
byte-exact: a capture in a new format gives what the oracle, the reference's chain or the same device call gives on the RGB image OpenCV would
build of it (tests/capture_formats_native.py: to_rgb)."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from oracle.pyref import P
from tests import automode_model as AM
from tests import capture_formats_native as CN
from tests import distorted_captures as DC
from tests import frames as F
from tests.test_capture_formats import reference_capture_chain
from tests.test_gpu_flood_verify import decoder_with
from tests.test_oracle_vs_ref import CAMERA_CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080

_cache = {}


def camera_rgb(synth):
    """the four CAMERA_CASES at 1080p as RGB captures, made once"""
    if "cams" not in _cache:
        payload, frames = F.clean_frames(synth, len(CAMERA_CASES), seed=90)
        _cache["cams"] = [F.camera_frame(frames[k], width=W, height=H, quad=q, background=bg, blur=bl) for k, (bg, q, bl) in enumerate(CAMERA_CASES)]
    return _cache["cams"]


def camera_set(synth, oracle, fmt):
    """-> (captures (4, bytes) in `fmt`, the RGB images OpenCV would build of them (4, h, w, 3)), made once per format"""
    if ("set", fmt) not in _cache:
        cams = np.ascontiguousarray(np.stack([CN.rgb_to_native(c, fmt) for c in camera_rgb(synth)]))
        seen = np.ascontiguousarray(np.stack([CN.to_rgb(oracle, c, W, H, fmt) for c in cams]))
        cams.setflags(write=False)
        seen.setflags(write=False)
        _cache[("set", fmt)] = (cams, seen)
    return _cache[("set", fmt)]


SIZES = [((1920, 1080), "3x3-streaming"), ((2608, 1700), "5x5-streaming"), ((1282, 978), "3x3-tiled-odd-width"), ((64, 40), "tiny"),
         ((4000, 2600), "9x9-tiled")]
PRE_CASES = [pytest.param(fmt, size, id=f"{fmt}-{name}") for fmt in CN.NATIVE for size, name in SIZES]
# an odd height: any implementation of 4:2:2 that shares chroma between rows fails here; an odd width too for the packed formats
PRE_CASES += [pytest.param(fmt, size, id=f"{fmt}-{size[0]}x{size[1]}") for fmt in CN.ANY_HEIGHT for size in ((1920, 1079), (1282, 977))]
PRE_CASES += [pytest.param(fmt, (1283, 977), id=f"{fmt}-1283x977") for fmt in (30, 40)]


@pytest.mark.parametrize("fmt,size", PRE_CASES)
def test_scan_preprocess(hip_decoder, oracle, fmt, size):
    w, h = size
    rng = np.random.default_rng(w + fmt)
    img = rng.integers(0, 256, (1, CN.capture_bytes(w, h, fmt)), dtype=np.uint8)
    img[0, : img.shape[1] // 2] //= 3                              # a dark half so that Otsu has something to find
    got, thr = hip_decoder.scan_preprocess(img, size=size, fmt=fmt)
    want = np.zeros((h, w), np.uint8)
    rgb = CN.to_rgb(oracle, img[0], w, h, fmt)
    assert thr[0] == oracle.co_scan_preprocess(P(rgb), w, h, P(want))
    assert (got[0] == want).all(), f"{(got[0] != want).sum()} pixels differ"


@pytest.mark.parametrize("fmt", CN.NATIVE)
def test_extract_batch(hip_decoder, synth, oracle, fmt):
    """status, corners and the deskewed frame == the oracle's Extractor on the RGB image; then corners that push part of the frame outside the
    capture (the warp's border path)"""
    cams, seen = camera_set(synth, oracle, fmt)
    status, corners, frames = hip_decoder.extract_batch(cams, size=(W, H), fmt=fmt)
    for k in range(len(cams)):
        want = np.zeros((1024, 1024, 3), np.uint8)
        c8 = (ctypes.c_float * 8)()
        rc = oracle.co_extract_fmt(P(seen[k]), W, H, 3, P(want), c8)
        assert status[k] == rc and rc in (1, 2)
        assert list(corners[k]) == list(c8)
        assert (frames[k] == want).all(), f"capture {k}: {(frames[k] != want).sum()} bytes differ"
    far = corners.copy()
    far[:, 0] -= 500; far[:, 1] -= 300; far[:, 6] += 450; far[:, 7] += 200
    desk = hip_decoder.deskew_batch(cams, far, size=(W, H), fmt=fmt)
    for k in range(len(cams)):
        want = np.zeros((1024, 1024, 3), np.uint8)
        oracle.co_deskew(P(seen[k]), W, H, far[k].ctypes.data_as(ctypes.POINTER(ctypes.c_float)), P(want))
        assert (desk[k] == want).all(), f"capture {k}: {(desk[k] != want).sum()} bytes differ"


@pytest.mark.parametrize("fmt", CN.NATIVE)
def test_chain_equals_the_references_chain_on_the_rgb_image(hip_decoder, synth, oracle, ref, fmt):
    """cimbar_hip_scan_extract_decode_batch_fmt(preprocess 1, colour correction 2) on captures in `fmt` against the reference's own
    cimbard_scan_extract_decode on their RGB images, capture by capture in order; host buffers, then device buffers"""
    cams, seen = camera_set(synth, oracle, fmt)
    batch = np.ascontiguousarray(np.concatenate([cams, CN.blank(W, H, fmt)[None]], 0))
    hip_decoder.reset_ccm()
    total, chunks, masks, status = hip_decoder.scan_extract_decode_batch(batch, preprocess=1, size=(W, H), fmt=fmt)
    ref.ref_reset_ccm()
    want_total = 0
    for k in range(len(batch)):
        rgb = seen[k] if k < len(seen) else CN.to_rgb(oracle, batch[k], W, H, fmt)
        r, buf = reference_capture_chain(ref, np.ascontiguousarray(rgb), W, H, 3)
        if r == -3:
            assert status[k] == 0 and masks[k] == 0 and not chunks[k].any()
            continue
        packed = np.concatenate([chunks[k][j] for j in range(12) if masks[k] >> j & 1] + [np.zeros(0, np.uint8)])
        assert packed.size == r and (packed == buf[:r]).all(), k
        want_total += r
    assert status[-1] == 0                                          # the blank capture
    assert total == want_total >= 7500
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.from_numpy(batch).to(dev)
    n = len(batch)
    d_chunks = torch.zeros((n, 7500), dtype=torch.uint8, device=dev)
    d_masks = torch.zeros((n,), dtype=torch.int32, device=dev)
    d_status = torch.zeros((n,), dtype=torch.int32, device=dev)
    hip_decoder.reset_ccm()
    hip_decoder.scan_extract_decode_device(d_in.data_ptr(), W, H, n, d_chunks.data_ptr(), d_masks.data_ptr(), d_status.data_ptr(), preprocess=1, stream=st, fmt=fmt)
    torch.cuda.synchronize()
    assert (d_chunks.cpu().numpy() == chunks.reshape(n, -1)).all() and (d_masks.cpu().numpy().astype(np.uint32) == masks).all()
    assert (d_status.cpu().numpy() == status).all()


@pytest.mark.parametrize("fmt", CN.YUV_NATIVE)
def test_warp_routes_agree(hip_decoder, synth, oracle, fmt):
    """the default route, the convert-ahead pass in several passes (16 MB of scratch: two 1080p captures per pass and an odd one left) and the
    conversion inside the warp kernel (CIMBAR_HIP_WARP_TWOPASS=0): the same status, corners and frames"""
    cams, _ = camera_set(synth, oracle, fmt)
    cams = np.ascontiguousarray(np.concatenate([cams, cams[:3]]))
    assert len(cams) % 2 == 1 and len(cams) >= 5
    status, corners, frames = hip_decoder.extract_batch(cams, size=(W, H), fmt=fmt)
    assert (status > 0).all()
    for env in ({"CIMBAR_HIP_WARP_SCRATCH_MB": "16"}, {"CIMBAR_HIP_WARP_TWOPASS": "0"}):
        d = decoder_with(env)
        try:
            s2, c2, f2 = d.extract_batch(cams, size=(W, H), fmt=fmt)
        finally:
            d.close()
        assert (s2 == status).all() and (c2 == corners).all() and (f2 == frames).all(), env


def undistort_rgb():
    if "ud" not in _cache:
        _cache["ud"] = [DC.distorted(640, 480, 0.006, 11), DC.distorted(640, 480, -0.004, 12)]
    return _cache["ud"]


@pytest.mark.parametrize("fmt", CN.NATIVE)
def test_undistort(hip_decoder, oracle, fmt):
    """cimbar_hip_undistort_batch_fmt with explicit parameters (k1 != 0, zeros at the border) and with calibration == the same call on the RGB images"""
    w, h = 640, 480
    caps = np.ascontiguousarray(np.stack([CN.rgb_to_native(c, fmt) for c in undistort_rgb()]))
    seen = np.ascontiguousarray(np.stack([CN.to_rgb(oracle, c, w, h, fmt) for c in caps]))
    params = [w / 3.0, 0, w / 2.0 + 3.5, 0, h / 3.0, h / 2.0 - 2.25, 0, 0, 1, 0.08, 0.01, 0, 0, 0]
    for p in (params, None):
        out, ok, k1 = hip_decoder.undistort_batch(caps, params=p, size=(w, h), fmt=fmt)
        want, wok, wk1 = hip_decoder.undistort_batch(seen, params=p)
        assert (ok == wok).all() and k1.tobytes() == wk1.tobytes()
        assert (out == want).all(), f"{(out != want).any(-1).sum()} pixels differ"
        if p is not None:
            assert (ok == 1).all() and (out != seen).any()


def test_undistort_composite_in_yuyv(hip_decoder, oracle):
    rgbs = [DC.distorted(W, H, 0.006, 11), DC.blank()]
    caps = np.ascontiguousarray(np.stack([CN.rgb_to_native(c, 422) for c in rgbs]))
    seen = np.ascontiguousarray(np.stack([CN.to_rgb(oracle, c, W, H, 422) for c in caps]))
    hip_decoder.reset_ccm()
    got = hip_decoder.scan_undistort_extract_decode_batch(caps, preprocess=1, size=(W, H), fmt=422)
    hip_decoder.reset_ccm()
    want = hip_decoder.scan_undistort_extract_decode_batch(seen, preprocess=1)
    assert got[0] == want[0]
    for g, w_ in zip(got[1:], want[1:]):
        assert (g == w_).all()


def three_captures(synth, oracle, fmt):
    cams, seen = camera_set(synth, oracle, fmt)
    return np.ascontiguousarray(cams[:3]), np.ascontiguousarray(seen[:3])


def test_auto_object_in_yuyv(oracle):
    from libcimbar_amd import AutoDecoder
    rgbs = [AM.capture(68, 700), AM.capture(66, 701), AM.capture(68, 702)]
    caps = np.ascontiguousarray(np.stack([CN.rgb_to_native(c, 422) for c in rgbs]))
    seen = np.ascontiguousarray(np.stack([CN.to_rgb(oracle, c, W, H, 422) for c in caps]))
    dec = AutoDecoder(0, [68, 66])
    try:
        got = dec.scan_extract_decode_batch_raw(caps, preprocess=1, size=(W, H), fmt=422)
        dec.reset_ccm()
        want = dec.scan_extract_decode_batch_raw(seen, preprocess=1)
    finally:
        dec.close()
    assert got[0] == want[0]
    for g, w_ in zip(got[1:], want[1:]):
        assert (g == w_).all()
    # (the sequential model, tests/automode_model.py, on these RGB images: the first capture's colours do not survive 4:2:2 without a carried
    # matrix, the mode-66 capture sets one, the third decodes in full)
    assert list(want[3]) == [0, 66, 68] and want[2][2] == 0xFFF


def test_combined_call_in_uyvy(hip_decoder, synth, oracle):
    caps, seen = three_captures(synth, oracle, 4221)
    hip_decoder.reset_ccm()
    got = hip_decoder.scan_extract_decode_batch_combined(caps, preprocess=1, size=(W, H), fmt=4221)
    hip_decoder.reset_ccm()
    want = hip_decoder.scan_extract_decode_batch_combined(seen, preprocess=1)
    assert got[0] == want[0]
    for g, w_ in zip(got[1:], want[1:]):
        assert (g == w_).all()
    assert (want[3] > 0).all()


def test_stitched_call_in_nv21(hip_decoder, synth, oracle):
    caps, seen = three_captures(synth, oracle, 21)
    hip_decoder.reset_ccm()
    got = hip_decoder.scan_extract_decode_batch_stitched(caps, preprocess=1, size=(W, H), fmt=21)
    hip_decoder.reset_ccm()
    want = hip_decoder.scan_extract_decode_batch_stitched(seen, preprocess=1)
    assert got[0] == want[0]
    for g, w_ in zip(got[1:], want[1:]):
        assert (g == w_).all()
    assert (want[3] > 0).all()


def test_dimensions_the_layouts_cannot_hold(hip_decoder):
    lib = D.load_library()
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(64 * 64, np.uint8)
    for fmt, w, h in ((422, 63, 64), (4221, 63, 64), (21, 63, 64), (21, 64, 63)):
        assert lib.cimbar_hip_scan_preprocess_fmt(hip_decoder._ctx, buf.ctypes.data, w, h, fmt, 1, D.MEM_HOST, out.ctypes.data, None, D.MEM_HOST, None) == -2, (fmt, w, h)
    for fmt in (422, 4221):                                         # an odd height is fine in 4:2:2
        assert lib.cimbar_hip_scan_preprocess_fmt(hip_decoder._ctx, buf.ctypes.data, 64, 63, fmt, 1, D.MEM_HOST, out.ctypes.data, None, D.MEM_HOST, None) == 0


def test_the_references_interface_keeps_the_references_meaning(synth):
    """libcimbar_recv_hip.so is the reference's C interface: 422 and 30 are no format get_rgb knows, so they are RGB8 there as they always were"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libcimbar_amd", "libcimbar_recv_hip.so"))
    img = np.ascontiguousarray(camera_rgb(synth)[0])
    lib.cimbard_configure_decode(68)
    bufs = {fmt: np.zeros(7500, np.uint8) for fmt in (3, 422, 30)}
    rets = {}

    def call(fmt):                                                  # (the decoder and its carried matrix are per calling thread: a fresh one each)
        rets[fmt] = lib.cimbard_scan_extract_decode(P(img), W, H, fmt, P(bufs[fmt]), bufs[fmt].size)
    for fmt in bufs:
        t = threading.Thread(target=call, args=(fmt,))
        t.start()
        t.join()
    assert rets[3] > 0
    for fmt in (422, 30):
        assert rets[fmt] == rets[3] and (bufs[fmt] == bufs[3]).all(), fmt
