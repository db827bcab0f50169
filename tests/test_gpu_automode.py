"""GPU: mode auto-detection (cimbar_hip_auto_scan_extract_decode_batch_fmt / AutoDecoder) bit-exact against the sequential model
(tests/automode_model.py): accepted mode, chunks, mask, status per capture and the carried matrix after the call.
The last tests walk k_auto_resolve past its first round of 1024 captures (resolve_case)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref
from tests import automode_model as AM
from tests import colour_cases as CC

pytestmark = pytest.mark.gpu

WEB = [66, 68, 67, 4]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cams():
    """mixed-mode 1080p captures: every mode, a blank one, a partly occluded mode-B one"""
    out = [AM.capture(m, 500 + k) for k, m in enumerate([68, 67, 66, 4, 8, 0, 68])]
    occl = out[-1].copy()
    occl[300:620, 700:1100] = 0
    out[-1] = occl
    return out


def check(dec, cams, fmt, cand, pre=1, cc=2, order=None, ccm=None):
    imgs = AM.to_format(cams, fmt)
    h, w = cams[0].shape[:2]
    want, ccm_after = AM.auto_batch(imgs, w, h, fmt, cand, ccm=ccm, preprocess=pre, cc=cc)
    total, slots, masks, modes, status = dec.scan_extract_decode_batch_raw(imgs, preprocess=pre, color_correction=cc, size=(w, h), fmt=fmt, order=order)
    expect_total = 0
    for f, (m, st, chunks, mask) in enumerate(want):
        assert modes[f] == m and masks[f] == mask and status[f] == st, (f, modes[f], m, masks[f], mask, status[f], st)
        fb = pyref.GEOMETRY[m][6] * pyref.GEOMETRY[m][3] if m else 0
        if m:
            assert (slots[f, :fb] == chunks.reshape(-1)).all(), f
            expect_total += bin(mask).count("1") * pyref.GEOMETRY[m][3]
        assert not slots[f, fb:].any(), f
    assert total == expect_total
    active, mat = dec.get_ccm()
    assert active == bool(ccm_after.active)
    if active:
        assert (mat.reshape(-1) == np.array(list(ccm_after.m), np.float32)).all()
    return want, ccm_after


@pytest.mark.parametrize("fmt", [3, 4, 12, 420])
def test_mixed_batch_every_format(cams, fmt):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    want, _ = check(dec, cams, fmt, WEB + [8])
    # (mode 8's eight colours do not survive 4:2:0 chroma: there the model and the device agree that nothing decodes)
    assert [w[0] for w in want][:5] == ([68, 67, 66, 4, 8] if fmt in (3, 4) else [68, 67, 66, 4, 0])


@pytest.mark.parametrize("cc", [0, 1, 2])
@pytest.mark.parametrize("pre", [1, -1])
def test_colour_correction_and_preprocess(cams, cc, pre):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    check(dec, cams, 3, WEB + [8], pre=pre, cc=cc)


@pytest.mark.parametrize("order", [[68], [8, 4, 66, 67, 68], [67, 4], [4, 66]])
def test_candidate_orders(cams, order):
    from libcimbar_amd import AutoDecoder
    dec = AutoDecoder(0, WEB + [8])
    check(dec, cams, 12, order, order=order)


def test_batch_sizes_and_the_carry_across_calls(cams):
    from libcimbar_amd import AutoDecoder
    rng = np.random.default_rng(3)
    big = [cams[i] for i in rng.integers(0, len(cams), 33)]
    dec = AutoDecoder(0, WEB)
    check(dec, big[:1], 3, WEB)
    dec.reset_ccm()
    _, ccm = check(dec, big, 3, WEB)
    # two calls = one call on their concatenation: the matrix crosses the call boundary
    dec.reset_ccm()
    _, ccm1 = check(dec, big[:20], 3, WEB)
    check(dec, big[20:], 3, WEB, ccm=ccm1)
    assert dec.get_ccm()[0] == bool(ccm.active)


def test_hundreds_of_captures_on_a_caller_stream(cams):
    import ctypes
    import torch
    from libcimbar_amd import AutoDecoder
    n = 300
    idx = np.arange(n) % len(cams)
    imgs = AM.to_format(cams, 12)
    h, w = cams[0].shape[:2]
    # the model over the real sequence of 300; an attempt's result depends only on (capture, matrix carried in), so repeats are looked up
    ccm, memo, want = pyref.CoCcm(), {}, []
    for f in range(n):
        key = (int(idx[f]), bytes(ccm))
        if key not in memo:
            r = AM.auto_decode(np.ascontiguousarray(imgs[idx[f]]), w, h, 12, WEB, ccm)
            memo[key] = (r, bytes(ccm))
        r, after = memo[key]
        ctypes.memmove(ctypes.addressof(ccm), after, ctypes.sizeof(ccm))
        want.append(r)
    dec = AutoDecoder(0, WEB)
    d_in = torch.from_numpy(imgs[idx].reshape(n, -1)).cuda()
    slots = torch.zeros((n, dec.slot), dtype=torch.uint8, device="cuda")
    masks = torch.zeros(n, dtype=torch.int32, device="cuda")
    modes = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        total = dec.scan_extract_decode_device(d_in.data_ptr(), w, h, n, slots.data_ptr(), masks.data_ptr(), modes.data_ptr(), status.data_ptr(),
                                               preprocess=1, fmt=12, stream=st.cuda_stream)
    st.synchronize()
    modes, masks, status, slots = modes.cpu().numpy(), masks.cpu().numpy().view(np.uint32), status.cpu().numpy(), slots.cpu().numpy()
    for f in range(n):
        m, s, ch, mk = want[f]
        assert modes[f] == m and status[f] == s and masks[f] == mk, f
        if m:
            assert (slots[f, :ch.size] == ch.reshape(-1)).all(), f
    assert total == sum(bin(int(x)).count("1") * (pyref.GEOMETRY[int(m)][3] if m else 0) for x, m in zip(masks, modes))
    active, mat = dec.get_ccm()
    assert active == bool(ccm.active) and (not active or (mat.reshape(-1) == np.array(list(ccm.m), np.float32)).all())


@pytest.mark.parametrize("mode", [68, 67, 66, 4, 8])
def test_single_candidate_equals_the_per_mode_entry_point(cams, mode):
    from libcimbar_amd import AutoDecoder, HipDecoder
    imgs = AM.to_format(cams, 3)
    h, w = cams[0].shape[:2]
    dec = AutoDecoder(0, [mode])
    total, slots, masks, modes, status = dec.scan_extract_decode_batch_raw(imgs, preprocess=1, size=(w, h), fmt=3)
    t2, c2, m2, s2 = HipDecoder(0, mode).scan_extract_decode_batch(imgs, preprocess=1, size=(w, h), fmt=3)
    assert total == t2 and (masks == m2).all()
    fb = c2[0].size
    for f in range(len(imgs)):
        assert (slots[f, :fb] == c2[f].reshape(-1)).all(), f
        assert modes[f] == (mode if m2[f] else 0)
        assert status[f] == s2[f]


def test_the_carry_across_modes():
    """a mode-68 capture under a colour cast derives a matrix from its fountain header; a later mode-4 capture under the same cast (legacy: no
    matrix of its own, its whole result is the colour pass) decodes with that matrix in force -- and decodes nothing after reset_ccm"""
    from libcimbar_amd import AutoDecoder
    gain = np.array([0.6, 1.0, 0.45])
    c68 = AM.capture(68, 0, frame=CC.cast(AM.mode_frame(68, 700), np.eye(3), gain))
    c4 = AM.capture(4, 0, frame=CC.cast(AM.mode_frame(4, 701), np.eye(3), gain))
    dec = AutoDecoder(0, WEB)
    want, ccm = check(dec, [c68, c4], 3, WEB)
    assert ccm.active and [w[0] for w in want] == [68, 4] and want[1][3] != 0
    dec.reset_ccm()
    alone, _ = check(dec, [c4], 3, WEB)
    assert alone[0][0] == 0 and alone[0][3] == 0          # the same capture without the carried matrix: nothing
    # ... and a context per mode (no matrix crossing modes) would not have decoded it either
    from libcimbar_amd import HipDecoder
    _, _, m4, _ = HipDecoder(0, 4).scan_extract_decode_batch(c4[None], preprocess=1)
    assert m4[0] == 0


def test_convergence_from_a_wrong_guess():
    """CIMBAR_HIP_AUTO_GUESS_FIRST=1 starts the settling loop from 'every capture accepted at its first candidate': the result must be the same"""
    code = ("import sys; sys.path.insert(0, %r); from tests import test_gpu_automode as T, automode_model as AM; "
            "from libcimbar_amd import AutoDecoder; "
            "cams = [AM.capture(m, 500 + k) for k, m in enumerate([68, 67, 66, 4, 8, 0, 68])]; "
            "[T.check(AutoDecoder(0, T.WEB + [8]), cams, 3, T.WEB + [8], cc=cc) for cc in (1, 2)]; print('ok')") % ROOT
    env = dict(os.environ, CIMBAR_HIP_AUTO_GUESS_FIRST="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- k_auto_resolve past its first round: one workgroup resolves 1024 captures a round and hands the newest deriving attempt (s_run) on
ROUND = 1024
RES_N = ROUND + 40
# three casts; a mode-B capture under one derives a matrix from its fountain header, a legacy mode-4 capture derives none and its whole
# result is the colour pass under the matrix in force: 4A decodes only with A's matrix, 4C with any but B's (checked on the model below)
GAINS = dict(A=(0.6, 1.0, 0.45), B=(1.0, 0.55, 0.7), C=(0.5, 0.7, 1.0))
RES_NAMES = ("68A", "68B", "66C", "4A", "4C", "blank")
DERIVING, QUIET = (0, 1, 2), (3, 4, 5)                  # indices into RES_NAMES: mode-B captures; legacy and blank ones
_res = {}


def resolve_inputs():
    """the distinct captures in format 12 and the two index sequences over them"""
    if not _res:
        def cap(mode, seed, gain):
            return AM.capture(mode, 0, frame=CC.cast(AM.mode_frame(mode, seed), np.eye(3), np.array(GAINS[gain])))
        cams = [cap(68, 700, "A"), cap(68, 702, "B"), cap(66, 703, "C"), cap(4, 701, "A"), cap(4, 705, "C"), AM.capture(0, 0)]
        rng = np.random.default_rng(11)
        quiet = lambda k: rng.choice(QUIET, k)                                  # noqa: E731
        a = rng.integers(0, len(cams), RES_N)
        # a: B's matrix from 1010, nothing derived up to 1022; 1023 derives A's under its own cast and 1024 (4A) lives on it; 1040 derives a
        # third matrix, C's, in the second round, and 1041 (4A) meets that one, not the first round's
        a[1005:] = quiet(RES_N - 1005)
        a[[1010, 1023, 1024, 1040, 1041, 1042]] = [1, 0, 3, 2, 3, 4]
        # b: B's matrix from 990, A's from 1000, and nothing derived from there to the end: the second round lives on the first round's last
        b = rng.integers(0, len(cams), RES_N)
        b[985:] = quiet(RES_N - 985)
        b[[990, 1000, 1024, 1030]] = [1, 0, 3, 3]
        _res.update(cams=cams, imgs=AM.to_format(cams, 12), seq=dict(a=a, b=b), memo={})
    return _res


def resolve_one(u, ccm_in, cand, cc):
    """capture u of resolve_inputs() with the matrix ccm_in (the bytes of a CoCcm) carried in -> (result, the bytes of the matrix after);
    an attempt's result depends only on (capture, matrix carried in), so repeats are looked up"""
    import ctypes
    r = resolve_inputs()
    key = (int(u), ccm_in, tuple(cand), cc)
    if key not in r["memo"]:
        ccm = pyref.CoCcm()
        ctypes.memmove(ctypes.addressof(ccm), ccm_in, ctypes.sizeof(ccm))
        h, w = r["cams"][0].shape[:2]
        res = AM.auto_decode(np.ascontiguousarray(r["imgs"][u]), w, h, 12, list(cand), ccm, cc=cc)
        r["memo"][key] = (res, bytes(ccm))
    return r["memo"][key]


def resolve_model(idx, cand, cc):
    """-> per capture (mode, status, chunks, mask), and the matrix in force before capture f (f = n: the one carried out)"""
    trace, want = [bytes(pyref.CoCcm())], []
    for u in idx:
        res, after = resolve_one(u, trace[-1], cand, cc)
        want.append(res)
        trace.append(after)
    return want, trace


def resolve_shapes(name, idx, cand, want, trace):
    """the hand-overs the sequence is there for, on the model's trace of the matrix in force (color_correction 2)"""
    differs = lambda x, y: x[0] != y[0] or x[3] != y[3] or (x[0] and not np.array_equal(x[2], y[2]))    # noqa: E731
    derived = [f for f in range(len(idx)) if trace[f + 1] != trace[f]]
    assert all(idx[f] in DERIVING for f in derived)
    if name == "a":
        # boundary hand-over: 1023 derives under a cast of its own, 1024 derives nothing and its result is that matrix's doing
        assert 1023 in derived and 1024 not in derived
        assert want[1024][0] == 4 and want[1024][3] != 0 and differs(want[1024], resolve_one(idx[1024], trace[0], cand, 2)[0])
        assert differs(want[1024], resolve_one(idx[1024], trace[1023], cand, 2)[0])
        # second-round order: 1040 derives a third matrix, and 1041 decodes under it, not under the first round's
        assert derived[-1] == 1040 and len({trace[1023], trace[1024], trace[1041]}) == 3 and trace[1042] == trace[1041]
        assert differs(want[1041], resolve_one(idx[1041], trace[1024], cand, 2)[0])
        assert derived[-1] >= ROUND                                        # the matrix carried out comes from the second round
    else:
        # long reach: the last derivation is capture 1000, and captures of the second round decode by it
        assert derived[-1] == 1000 and trace[1001] != trace[1000] and all(u in QUIET for u in idx[1001:])
        reach = [f for f in range(ROUND, len(idx)) if want[f][0] and differs(want[f], resolve_one(idx[f], trace[1000], cand, 2)[0])]
        assert 1024 in reach and 1030 in reach
        assert derived[-1] < ROUND                                         # ... and so does the matrix carried out


def resolve_case(name, cc=2, order=None):
    """one sequence through the device (the captures gathered there from the six distinct ones) against the model"""
    import torch
    from libcimbar_amd import AutoDecoder
    r = resolve_inputs()
    idx = r["seq"][name]
    cand = WEB if order is None else order
    want, trace = resolve_model(idx, cand, cc)
    if cc == 2:
        resolve_shapes(name, idx, cand, want, trace)
    n = len(idx)
    h, w = r["cams"][0].shape[:2]
    dec = AutoDecoder(0, WEB)
    d_in = torch.from_numpy(r["imgs"]).cuda()[torch.from_numpy(idx).cuda()].reshape(n, -1)
    slots = torch.zeros((n, dec.slot), dtype=torch.uint8, device="cuda")
    masks, modes, status = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    total = dec.scan_extract_decode_device(d_in.data_ptr(), w, h, n, slots.data_ptr(), masks.data_ptr(), modes.data_ptr(), status.data_ptr(),
                                           preprocess=1, color_correction=cc, fmt=12, order=order)
    torch.cuda.synchronize()
    modes, masks, status, slots = modes.cpu().numpy(), masks.cpu().numpy().view(np.uint32), status.cpu().numpy(), slots.cpu().numpy()
    for f in range(n):
        m, s, ch, mk = want[f]
        assert modes[f] == m and status[f] == s and masks[f] == mk, (f, modes[f], m, status[f], s, hex(int(masks[f])), hex(mk))
        fb = ch.size if m else 0
        if m:
            assert (slots[f, :fb] == ch.reshape(-1)).all(), f
        assert not slots[f, fb:].any(), f
    assert total == sum(bin(int(x)).count("1") * (pyref.GEOMETRY[int(m)][3] if m else 0) for x, m in zip(masks, modes))
    carried = pyref.CoCcm.from_buffer_copy(trace[-1])
    active, mat = dec.get_ccm()
    assert active == bool(carried.active) and (not active or (mat.reshape(-1) == np.array(list(carried.m), np.float32)).all())


@pytest.mark.parametrize("name,cc,order", [("a", 2, None), ("b", 2, None), ("b", 1, None), ("a", 2, [4, 68, 66, 67])],
                         ids=["a-cc2", "b-cc2", "b-cc1", "a-cc2-reordered"])
def test_resolve_across_1024_captures(name, cc, order):
    resolve_case(name, cc, order)


def test_resolve_across_1024_captures_from_a_wrong_guess():
    code = ("import sys; sys.path.insert(0, %r); from tests import test_gpu_automode as T; T.resolve_case('a'); print('ok')") % ROOT
    env = dict(os.environ, CIMBAR_HIP_AUTO_GUESS_FIRST="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
