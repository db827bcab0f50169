"""GPU: the erasure retry of the stitched decode (cimbar_hip_set_stitch_erasure -> k_stitch_erasure, k_stitch_colour_erasure) on the four-capture
batches of tests/stitch_erasure_cases.py (tests/test_stitch_erasure_model.py vets them on the CPU), modes 68 / 67 / 66 unless noted.

1. Setting off: a context that never heard of the setting and one that has it off give byte-equal outputs, whatever the erasure settings; the
   new taps are EINVAL.
2. On equals the model: tests/stitch_erasure_model.py fed with the device's own taps (symbols, colours, drift, bit planes, flood flags,
   matrices, stitched cells, tear records) gives smasks, schunks, TAP_STITCH_DISTANCE and TAP_STITCH_COLOUR_MARGIN bit for bit, in every case
   of the set; B's slot (and Cd's) comes back with the full mask and the payload where the off run does not.
3. Matrix: each retry alone and both; sym_distance 1 / 6 / 64 x max_erasures default / 1 / 0; axis 1 (in the case set); strips 4 on a slanted
   tear. Everything the retry must not touch equals the off run: per-capture chunks and masks, the carried matrix, tear records, line
   counts, stitched cells, TAP_RS_OK.
4. Device outputs over poisoned buffers on a caller's stream; chunks of the off mask byte-identical, slots of chunks still missing zero,
   slots that are not live zero; modes 4 and 8 refuse the setter; a stitched-stream sequence is the same with the setting on.
5. The capture path: one 1280 x 720 case in format 3 with the damaged B.
6. Every chunk in every mask of every test is that chunk of a frame shown (`stitch_erasure_cases.genuine`, asserted wherever a mask is produced).
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import frames as F
from tests import stitch_cases as SC
from tests import stitch_erasure_cases as S
from tests import stitch_erasure_model as SE
from tests import stitch_model as SM
from tests import stitch_strips_cases as SSC
from tests import stitch_strips_model as SSM
from tests import symbol_erasure_model as M

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module", params=S.MODES)
def MODE(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return request.param


def _dec(mode, t_sym=S.T_SYM, colour_margin=S.MARGIN, sym_max=-1, col_max=-1, on=True, strips=1):
    d = D.HipDecoder(0, mode)
    d.set_erasure_decode(t_sym, -1, sym_max)
    d.set_colour_erasure_decode(colour_margin, col_max)
    d.set_stitch_strips(strips)
    if on is not None:
        d.set_stitch_erasure(on)
    return d


def _run(dec, caps, axis, strips=1):
    """one host-output call and everything the comparisons need of it"""
    n = len(caps)
    dec.reset_ccm()
    cand, chunks, masks, schunks, smasks, tears = dec.decode_batch_stitched(caps, axis=axis)
    out = dict(cand=cand, chunks=chunks, masks=masks, schunks=schunks, smasks=smasks, tears=tears, ccm=dec.get_ccm(),
               lines=dec.tap_stitch_lines(n, axis), cells=dec.tap(D.TAP_STITCH_CELLS, n), rs_ok=dec.tap(D.TAP_RS_OK, n))
    if strips > 1:
        out["strips"] = dec.tap_stitch_strips(n, strips)
    return out


def _untouched(on, off):
    for key in ("chunks", "masks", "tears", "lines", "cells", "rs_ok", "cand"):
        assert np.array_equal(on[key], off[key]), key
    assert on["ccm"][0] == off["ccm"][0] and np.array_equal(on["ccm"][1], off["ccm"][1])
    if "strips" in off:
        assert np.array_equal(on["strips"], off["strips"])


def _model(dec, mode, caps, axis, on, off, t_sym, colour_margin, sym_max=-1, col_max=-1):
    """the model over the device's own taps of the call `on` describes -> (smasks, schunks, distances, margins)"""
    n = len(caps)
    sym, drift, plane = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_BITPLANE, n)
    flood, ccm = dec.tap(D.TAP_FLOOD, n), dec.tap(D.TAP_CCM, n)
    # the decision is the stitch model's, over the device's own per-capture cells
    col = dec.tap(D.TAP_COLORS, n)
    if "strips" in on:
        wt, ws, _, wcells = SSM.stitch_batch(mode, sym, col, axis, on["strips"].shape[1])
        assert np.array_equal(ws, on["strips"])
    else:
        wt, _, wcells = SM.stitch_batch(mode, sym, col, axis)
    assert np.array_equal(wt, on["tears"]) and np.array_equal(wcells, on["cells"])
    dists = [M.cell_distances(mode, plane[k], sym[k], drift[k], bool(flood[k])) for k in range(n)]
    margs = [SE.capture_margins(mode, caps[k], drift[k], bool(flood[k]), ccm[k]) for k in range(n)] if colour_margin > 0 else None
    return SE.retry_batch(mode, axis, on["tears"], on["cells"], dists, margs, off["smasks"], off["schunks"], on.get("strips"),
                          t_sym=t_sym, colour_margin=colour_margin, sym_max=sym_max, col_max=col_max)


def _taps(dec, n, t_sym, colour_margin):
    geo = dec.geo
    if t_sym > 0:
        d = dec.tap_stitch_distance(n)
    else:
        with pytest.raises(D.CimbarHipError):
            dec.tap_stitch_distance(n)
        d = np.full((2 * (n - 1), geo.NCELLS), SE.DIST_SKIPPED, np.uint8)
    if colour_margin > 0:
        g = dec.tap_stitch_colour_margin(n)
    else:
        with pytest.raises(D.CimbarHipError):
            dec.tap_stitch_colour_margin(n)
        g = np.full((2 * (n - 1), geo.NCELLS), SE.MARGIN_SKIPPED, np.uint32)
    return d, g


def _compare(mode, caps, axis, shown, t_sym=S.T_SYM, colour_margin=S.MARGIN, sym_max=-1, col_max=-1, strips=1, what=""):
    """off run, on run, the model; asserts parity and what must stay untouched -> (on, off)"""
    n = len(caps)
    d_off = _dec(mode, t_sym, colour_margin, sym_max, col_max, False, strips)
    d_on = _dec(mode, t_sym, colour_margin, sym_max, col_max, True, strips)
    try:
        off = _run(d_off, caps, axis, strips)
        on = _run(d_on, caps, axis, strips)
        _untouched(on, off)
        wm, wc, wd, wg = _model(d_on, mode, caps, axis, on, off, t_sym, colour_margin, sym_max, col_max)
        gd, gg = _taps(d_on, n, t_sym, colour_margin)
    finally:
        d_off.close()
        d_on.close()
    for g in range(2 * (n - 1)):
        assert int(on["smasks"][g]) == int(wm[g]), f"{what}slot {g}: mask {int(on['smasks'][g]):#x}, model {int(wm[g]):#x}, off {int(off['smasks'][g]):#x}"
        assert np.array_equal(on["schunks"][g], wc[g]), f"{what}slot {g}: chunks"
        assert np.array_equal(gd[g], wd[g]), f"{what}slot {g}: TAP_STITCH_DISTANCE"
        assert np.array_equal(gg[g], wg[g]), f"{what}slot {g}: TAP_STITCH_COLOUR_MARGIN"
    _superset(mode, on, off, shown, what)
    return on, off


def _superset(mode, on, off, shown, what=""):
    geo = geometry.for_mode(mode)
    for g in range(len(off["smasks"])):
        m0, m1 = int(off["smasks"][g]), int(on["smasks"][g])
        assert m0 & ~m1 == 0, f"{what}slot {g}: {m0:#x} -> {m1:#x}"
        for j in range(geo.CHUNKS_PER_FRAME):
            if (m0 >> j) & 1:
                assert np.array_equal(on["schunks"][g, j], off["schunks"][g, j]), f"{what}slot {g} chunk {j} rewritten"
    live = np.repeat(on["tears"][:, 0] >= 0, 2)
    assert not on["smasks"][~live].any() and not on["schunks"][~live].any(), what
    bad = S.genuine(mode, shown, on["smasks"], on["schunks"])
    assert bad is None, what + bad
    bad = S.genuine(mode, shown, off["smasks"], off["schunks"])
    assert bad is None, what + bad


def test_setting_off_equals_a_context_without_it(MODE):
    caps, shown, where = S.batch(MODE, S.TARGET)
    n = len(caps)
    plain, off = _dec(MODE, on=None), _dec(MODE, on=False)
    try:
        assert plain.get_stitch_erasure() == 0 and off.get_stitch_erasure() == 0
        a, b = _run(plain, caps, S.TARGET[1]), _run(off, caps, S.TARGET[1])
        _untouched(a, b)
        assert np.array_equal(a["smasks"], b["smasks"]) and np.array_equal(a["schunks"], b["schunks"])
        for dec in (plain, off):
            with pytest.raises(D.CimbarHipError):
                dec.tap_stitch_distance(n)
            with pytest.raises(D.CimbarHipError):
                dec.tap_stitch_colour_margin(n)
        off.set_stitch_erasure(True)
        assert off.get_stitch_erasure() == 1
    finally:
        plain.close()
        off.close()
    assert int(a["smasks"][where["b"]]) != geometry.for_mode(MODE).FULL_MASK


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_on_equals_the_model(MODE, case):
    geo = geometry.for_mode(MODE)
    caps, shown, where = S.batch(MODE, case)
    pay = S.frames_of(MODE)["pay"]
    on, off = _compare(MODE, caps, case[1], shown)
    b = where["b"]
    assert int(off["smasks"][b]) != geo.FULL_MASK and int(on["smasks"][b]) == geo.FULL_MASK, (hex(int(off["smasks"][b])), hex(int(on["smasks"][b])))
    assert (on["schunks"][b].reshape(-1) == pay["B"]).all()
    if where["cd"] is not None:
        cd = where["cd"]
        assert int(off["smasks"][cd]) != geo.FULL_MASK and int(on["smasks"][cd]) == geo.FULL_MASK
        assert (on["schunks"][cd].reshape(-1) == pay["Cd"]).all()
        assert int(off["smasks"][where["complete"]]) == geo.FULL_MASK
    assert not (on["tears"][[g // 2 for g in where["dead"]], 0] >= 0).any()


@pytest.mark.parametrize("armed", ["symbol", "colour"])
def test_each_retry_alone(MODE, armed):
    geo = geometry.for_mode(MODE)
    caps, shown, where = S.batch(MODE, S.TARGET)
    t_sym, margin = (S.T_SYM, 0) if armed == "symbol" else (0, S.MARGIN)
    on, off = _compare(MODE, caps, S.TARGET[1], shown, t_sym=t_sym, colour_margin=margin, what=armed + ": ")
    symc = geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)
    kind = (1 << symc) - 1 if armed == "symbol" else geo.FULL_MASK & ~((1 << symc) - 1)
    gained = int(on["smasks"][where["b"]]) & ~int(off["smasks"][where["b"]])
    assert gained and gained & ~kind == 0, hex(gained)


@pytest.mark.parametrize("sym_max", [-1, 1, 0])
@pytest.mark.parametrize("t_sym", [1, 6, 64])
def test_settings_matrix(MODE, t_sym, sym_max):
    caps, shown, _ = S.batch(MODE, S.TARGET)
    _compare(MODE, caps, S.TARGET[1], shown, t_sym=t_sym, sym_max=sym_max, col_max=sym_max, what=f"t_sym {t_sym} max_erasures {sym_max}: ")


def test_strips_on_a_slanted_tear(MODE):
    f = S.frames_of(MODE)
    rise, gap, blend = SSC.SLANTS[1]
    p1, p2, rise_px = SSC.slant_pixels(MODE, 0, rise, gap)
    t1, t2 = SSC.slanted_pair(f["A"], f["B"], f["Cd"], 0, p1, p2, 0, rise_px, blend)
    caps = np.stack([f["A"], t1, t2, f["Cd"]])
    on, off = _compare(MODE, caps, 0, ("A", "B", "Cd"), strips=4, what="strips 4: ")
    assert on["tears"][1, 0] >= 0 and len({int(s) for s in on["strips"][1, :, 2]}) > 1, on["strips"][1].tolist()
    assert (on["smasks"] != off["smasks"]).any()


def test_device_outputs_on_a_callers_stream(MODE):
    geo = geometry.for_mode(MODE)
    caps, shown, where = S.batch(MODE, S.TARGET)
    n, axis = len(caps), S.TARGET[1]
    dev = torch.device("cuda", 0)
    ref, dec = _dec(MODE), _dec(MODE)
    try:
        want = _run(ref, caps, axis)
        d_in = torch.from_numpy(np.ascontiguousarray(caps)).to(dev)
        mk = lambda shape, dt: torch.full(shape, POISON if dt == torch.uint8 else -0x5A5A5A5B, dtype=dt, device=dev)
        chunks, masks = mk((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((n,), torch.int32)
        schunks, smasks = mk((2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK), torch.uint8), mk((2 * (n - 1),), torch.int32)
        tears = mk((n - 1, 4), torch.int32)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        dec.reset_ccm()
        with torch.cuda.stream(stream):
            rc = dec.decode_batch_stitched_device(d_in.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(),
                                                  tears.data_ptr(), axis=axis, stream=stream.cuda_stream)
        stream.synchronize()
        assert rc == 0
        assert np.array_equal(schunks.cpu().numpy(), want["schunks"]) and np.array_equal(smasks.cpu().numpy().view(np.uint32), want["smasks"])
        assert np.array_equal(chunks.cpu().numpy(), want["chunks"]) and np.array_equal(tears.cpu().numpy(), want["tears"])
        assert np.array_equal(dec.tap_stitch_distance(n), ref.tap_stitch_distance(n))
        assert np.array_equal(dec.tap_stitch_colour_margin(n), ref.tap_stitch_colour_margin(n))
        assert int(want["smasks"][where["b"]]) == geo.FULL_MASK
        # after a batch of another kind the taps describe nothing
        dec.decode_batch(caps[:1])
        with pytest.raises(D.CimbarHipError):
            dec.tap_stitch_distance(n)
    finally:
        ref.close()
        dec.close()


@pytest.mark.parametrize("mode", [4, 8])
def test_legacy_modes_refuse_the_setter(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dec = D.HipDecoder(0, mode)
    try:
        with pytest.raises(D.CimbarHipError):
            dec.set_stitch_erasure(True)
        dec.set_stitch_erasure(False)
        assert dec.get_stitch_erasure() == 0
    finally:
        dec.close()


def test_stitched_stream_is_not_affected(MODE):
    caps, shown, _ = S.batch(MODE, S.TARGET)
    axis = S.TARGET[1]
    got = []
    for on in (False, True):
        dec = _dec(MODE, on=on)
        try:
            seq = [dec.decode_batch_stitched_stream(part, axis=axis) for part in (caps[:1], caps[1:3], caps[3:])]
            with pytest.raises(D.CimbarHipError):
                dec.tap_stitch_distance(1)
            got.append(seq)
        finally:
            dec.close()
    for a, b in zip(*got):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_capture_path():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mode, axis, direction = 68, 0, 0
    geo = geometry.for_mode(mode)
    f = S.frames_of(mode)
    p1, p2 = SC.tear_pixels(mode, axis, "across")
    t1, t2 = SC.torn_pair(f["A"], f["B"], f["C"], axis, p1, p2, direction)
    quad = ((285, 4), (995, 8), (280, 715), (1000, 710))
    cams = np.ascontiguousarray(np.stack([F.camera_frame(s, width=1280, height=720, quad=quad, background=0) for s in (f["A"], t1, t2, f["C"])]))
    res = []
    for on in (False, True):
        dec = _dec(mode, on=on)
        try:
            cand, chunks, masks, status, schunks, smasks, tears = dec.scan_extract_decode_batch_stitched(cams, axis=axis, preprocess=1, size=(1280, 720), fmt=3)
            res.append(dict(chunks=chunks, masks=masks, status=status, schunks=schunks, smasks=smasks, tears=tears))
        finally:
            dec.close()
    off, on = res
    assert (on["status"] > 0).all() and on["tears"][1, 0] >= 0, (on["status"].tolist(), on["tears"].tolist())
    for key in ("chunks", "masks", "status", "tears"):
        assert np.array_equal(on[key], off[key]), key
    print("capture path: smasks off", [hex(int(m)) for m in off["smasks"]], "on", [hex(int(m)) for m in on["smasks"]])
    _superset(mode, on, off, ("A", "B", "C"), "capture path: ")
    slot = 2 + direction
    payB = f["pay"]["B"].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    for j in range(geo.CHUNKS_PER_FRAME):
        if (int(on["smasks"][slot]) >> j) & 1:
            assert np.array_equal(on["schunks"][slot, j], payB[j]), j
