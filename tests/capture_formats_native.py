"""Captures in the pixel formats of native receivers (include/cimbar_hip.h, enum cimbar_hip_format): NV21 (21), YUYV (422), UYVY (4221), BGR (30)
and BGRA (40). Test-side manufacture, and the RGB image OpenCV would build of such a capture -- worked out from what the oracle already pins for
NV12 (co_capture_to_rgb(..., 12)), since OpenCV runs every YUV layout through the same fixed-point BT.601 arithmetic [assumed-OpenCV]."""
import numpy as np

from oracle.pyref import P

NATIVE = (21, 422, 4221, 30, 40)
YUV_NATIVE = (21, 422, 4221)         # the ones with a convert-ahead route in front of the warp
ANY_HEIGHT = (422, 4221, 30, 40)     # (21 needs an even height)
CV_CODE = {21: 92, 422: 115, 4221: 107, 30: 4, 40: 3}   # COLOR_YUV2RGB_NV21, _YUY2, _UYVY, COLOR_BGR2RGB, COLOR_BGRA2RGB


def capture_bytes(w, h, fmt):
    return {21: w * h * 3 // 2, 422: w * h * 2, 4221: w * h * 2, 30: w * h * 3, 40: w * h * 4}[fmt]


def _nv12_to_rgb(oracle, nv12, w, h):
    out = np.zeros((h, w, 3), np.uint8)
    assert oracle.co_capture_to_rgb(P(np.ascontiguousarray(nv12)), w, h, 12, P(out)) == 0
    return out


def to_rgb(oracle, img, w, h, fmt):
    """the (h, w, 3) RGB image cv::cvtColor makes of one capture in `fmt`"""
    img = np.ascontiguousarray(img, np.uint8).reshape(-1)
    assert img.size == capture_bytes(w, h, fmt)
    if fmt == 21:                                   # NV12 with the bytes of each chroma pair exchanged
        nv12 = img.copy()
        c = nv12[w * h:].reshape(-1, 2)
        c[:] = c[:, ::-1].copy()
        return _nv12_to_rgb(oracle, nv12, w, h)
    if fmt in (422, 4221):
        # an NV12 image of height 2h: every luma row twice, chroma row r = the (U, V) pairs of row r. Its 2x2 sharing then IS the 4:2:2 rule (a pair
        # serves two horizontally adjacent pixels of one row), which the two equal output rows show.
        g = img.reshape(h, w // 2, 4)
        y0, u, y1, v = (0, 1, 2, 3) if fmt == 422 else (1, 0, 3, 2)
        luma = np.stack([g[..., y0], g[..., y1]], -1).reshape(h, w)
        chroma = np.stack([g[..., u], g[..., v]], -1).reshape(h, w)
        nv12 = np.concatenate([np.repeat(luma, 2, axis=0).reshape(-1), chroma.reshape(-1)])
        rgb2 = _nv12_to_rgb(oracle, nv12, w, 2 * h)
        assert (rgb2[0::2] == rgb2[1::2]).all()
        return np.ascontiguousarray(rgb2[0::2])
    ch = 3 if fmt == 30 else 4
    return np.ascontiguousarray(img.reshape(h, w, ch)[..., 2::-1])      # B, G, R(, A) -> R, G, B


def rgb_to_native(rgb, fmt, alpha=255):
    """(h, w, 3) uint8 -> flat uint8 capture in `fmt`: the BT.601 limited-range forward conversion of tests/capture_formats.py, chroma averaged over
    2x2 blocks for NV21 and over horizontal pairs only for 4:2:2"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    if fmt == 30:
        return np.ascontiguousarray(rgb[..., ::-1]).reshape(-1)
    if fmt == 40:
        out = np.empty((h, w, 4), np.uint8)
        out[..., :3] = rgb[..., ::-1]
        out[..., 3] = alpha
        return out.reshape(-1)
    f = rgb.astype(np.float64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    if fmt == 21:
        assert w % 2 == 0 and h % 2 == 0
        sub = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
        return np.concatenate([q(y).reshape(-1), np.stack([q(sub(v)), q(sub(u))], -1).reshape(-1)])
    assert fmt in (422, 4221) and w % 2 == 0
    sub = lambda c: c.reshape(h, w // 2, 2).mean(axis=2)
    yq, uq, vq = q(y).reshape(h, w // 2, 2), q(sub(u)), q(sub(v))
    planes = [yq[..., 0], uq, yq[..., 1], vq] if fmt == 422 else [uq, yq[..., 0], vq, yq[..., 1]]
    return np.stack(planes, -1).reshape(-1)


def blank(w, h, fmt):
    """a capture with nothing in it (black)"""
    if fmt in (30, 40):
        return np.zeros(capture_bytes(w, h, fmt), np.uint8)
    return rgb_to_native(np.zeros((h, w, 3), np.uint8), fmt)
