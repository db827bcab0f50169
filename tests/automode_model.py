"""Mode auto-detection, the sequential model: for each capture in batch order, the candidates in the caller's order, each one extract +
Decoder::decode_fountain in that mode (the oracle built for the mode), until one delivers a chunk -- with ONE carried colour-correction matrix
(a single CoCcm) shared by every mode, as the reference's thread_local one is (CimbDecoder.cpp:69-73; cimbard_configure_decode leaves it alone,
cimbar_recv_js.cpp:272-288). What cimbar_hip_auto_scan_extract_decode_batch_fmt must compute."""
import numpy as np

from oracle import pyref
from oracle.pyref import P
from tests import capture_formats as CF
from tests import frames as F

# a placement per mode that its captures decode under (tests/test_gpu_modes.py)
QUADS = {68: ((500, 40), (1480, 70), (470, 1030), (1500, 1000)), 67: ((300, 150), (1600, 170), (290, 930), (1620, 915)),
         66: ((400, 60), (1500, 75), (395, 1010), (1510, 1000)), 4: ((500, 40), (1480, 70), (470, 1030), (1500, 1000)),
         8: ((500, 40), (1480, 70), (470, 1030), (1500, 1000))}


def mode_frame(mode, seed):
    from libcimbar_amd import framegen
    synth = framegen.FrameSynth("cpu", mode)
    _, frames = F.clean_frames(synth, 1, seed=seed)
    return np.asarray(frames[0])


def capture(mode, seed, background=40, frame=None):
    """a 1080p RGB capture of one frame of `mode` (0: a blank capture)"""
    if mode == 0:
        return np.full((1080, 1920, 3), background, np.uint8)
    fr = mode_frame(mode, seed) if frame is None else frame
    return F.camera_frame(fr, quad=QUADS[mode], background=background)


def auto_decode(img, w, h, fmt, candidates, ccm, preprocess=1, cc=2):
    """one capture through the loop -> (mode, status, chunks or None, mask); `ccm` (pyref.CoCcm) is carried in place"""
    status0 = None
    for m in candidates:
        g = pyref.GEOMETRY[m]
        frame = np.zeros((g[1], g[0], 3), np.uint8)
        st = pyref.oracle_lib(m).co_extract_fmt(P(img), w, h, fmt, P(frame), None)
        if status0 is None:
            status0 = st
        if st <= 0:                  # no frame: every mode's decode returns -3 and touches nothing (cimbar_recv_js.cpp:168-172)
            return 0, status0, None, 0
        pre = preprocess if preprocess in (0, 1) else (1 if st == 2 else 0)
        r, chunks, mask, ccm = pyref.oracle_decode(frame, pre, cc, ccm, mode=m)
        if r > 0:
            return m, st, chunks.copy(), mask
    return 0, status0, None, 0


def auto_batch(imgs, w, h, fmt, candidates, ccm=None, preprocess=1, cc=2):
    """captures in format `fmt` -> list of (mode, status, chunks, mask), the CoCcm after"""
    ccm = pyref.CoCcm() if ccm is None else ccm
    out = [auto_decode(np.ascontiguousarray(img), w, h, fmt, candidates, ccm, preprocess, cc) for img in imgs]
    return out, ccm


def packed(chunks, mask, mode):
    """what escrow_buffer_writer makes of a result: the delivered chunks front to back"""
    if chunks is None:
        return np.zeros(0, np.uint8)
    per = pyref.GEOMETRY[mode][6]
    return np.concatenate([chunks[j] for j in range(per) if mask >> j & 1] + [np.zeros(0, np.uint8)])


def to_format(cams, fmt):
    return np.stack([CF.rgb_to_format(c, fmt) for c in cams])
