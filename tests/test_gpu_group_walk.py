"""GPU: the group walks past their first step of 64 captures (csrc/combine.hip.inc k_group_walk with groups_in == nullptr and
k_group_walk_stream), on the batches of tests/group_walk_cases.py in mode 66, the smallest frame. tests/test_group_walk_cases.py shows on the
CPU that these batches hold every shape a hand-over between steps can get wrong and that forgetting any one carried variable changes their
result; here the device has to get them right. Every comparison is exact.

1. decode_batch_combined, automatic grouping, up to 200 captures at max_group 1, 3, the default and 8:
   groups and the count = tests/combine_model.group_captures on the call's own symbol and colour taps (and = the grouping the CPU test
   vetted); gchunks / gmasks = those of a call on a fresh context with groups= the model's ids (the branch test_erasure_superset_and_no_wrong_chunk
   pins at 200 captures); per-capture chunks, masks and the carried matrix = decode_batch's; the groups that straddle a step, made of
   the disjoint-damage pairs of test_recovery_from_disjoint_damage, deliver the whole payload though no member does.
2. scan_extract_decode_batch_combined on the same run list as 1280x720 captures with blank ones at 63, 64, 127 and 190 .. 193: the same
   assertions with usable = the returned status.
3. decode_batch_combined_stream over sequences of calls whose virtual batches (carried members + the call's captures) cross 64 and 128:
   per call groups, n_closed and gsizes = tests/combine_stream_model.StreamModel fed the call's taps; over the sequence the closed groups,
   the per-capture outputs and the matrix = ONE plain combined call on the whole batch (test_split_equivalence's assertions).
4. The same through scan_extract_decode_batch_combined_stream, where calls also end on blank captures.
"""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import geometry
from tests import capture_formats as CF
from tests import combine_model as CM
from tests import combine_stream_model as SM
from tests import frames as F
from tests import group_walk_cases as GW
from tests.test_gpu_combine_stream import _check_call_shape, _closed

pytestmark = pytest.mark.gpu

MODE = 66
AGREE = GW.AGREE_3
FMT = 3


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def RENDERED(gpu):
    return GW.rendered(MODE)


@pytest.fixture(scope="module")
def CAPTURED(gpu):
    """the distinct captures as 1280x720 camera captures (white discs: large black or noise discs can make the anchor search fail), the
    blank one last; and CAPTURE_RUNS with CAPTURE_BLANKS as indices into them"""
    uniq, _ = GW.rendered(MODE, kinds=("white",))
    w, h = GW.CAPTURE_SIZE
    cams = [F.camera_frame(f, width=w, height=h, quad=GW.CAPTURE_QUAD, background=96) for f in uniq]
    cams.append(np.full_like(cams[0], 96))
    raw = np.stack([CF.rgb_to_format(c, FMT) for c in cams])
    idx = GW.unique_index(GW.CAPTURE_RUNS)
    idx[list(GW.CAPTURE_BLANKS)] = len(cams) - 1
    return raw, idx


def _batch(rendered, name):
    return rendered[0][GW.unique_index(GW.RUN_LISTS[name])]


def _synthetic_groups(name, cap, usable=None):
    sym, col = GW.synthetic_cells(GW.RUN_LISTS[name])
    return CM.group_captures(sym, col, usable=usable, min_agree_permille=AGREE, max_group=cap)


def _same_ccm(a, b):
    return a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


# ------------------------------------------------------------------------------------------------ 1. automatic grouping, rendered frames
@pytest.mark.parametrize("name", list(GW.RUN_LISTS))
def test_automatic_grouping_across_steps(RENDERED, name):
    geo = geometry.for_mode(MODE)
    batch = _batch(RENDERED, name)
    payload = RENDERED[1]
    n = len(batch)
    frame, _, _ = GW.expand(GW.RUN_LISTS[name])
    plain = D.HipDecoder(0, MODE)
    try:
        _, rchunks, rmasks = plain.decode_batch(batch)
        rccm = plain.get_ccm()
    finally:
        plain.close()
    for cap in [c for nm, c in GW.WALK_CASES if nm == name]:
        auto, given = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
        try:
            ng, chunks, masks, groups, gchunks, gmasks = auto.decode_batch_combined(batch, min_agree_permille=AGREE, max_group=cap)
            sym, col = auto.tap(D.TAP_SYMBOLS, n), auto.tap(D.TAP_COLORS, n)
            want = CM.group_captures(sym, col, min_agree_permille=AGREE, max_group=cap)
            assert want.tolist() == _synthetic_groups(name, cap).tolist(), cap            # the batch behaves as the CPU test vetted it
            assert groups.tolist() == want.tolist(), (cap, np.flatnonzero(groups != want)[:10])
            assert ng == CM.n_groups(want)
            assert (auto.tap(D.TAP_GROUPS, n) == groups).all()
            assert (chunks == rchunks).all() and (masks == rmasks).all() and _same_ccm(auto.get_ccm(), rccm)
            g_ng, _, _, g_groups, g_gchunks, g_gmasks = given.decode_batch_combined(batch, groups=want, max_group=cap)
            assert g_ng == ng and g_groups.tolist() == want.tolist()
            assert (gmasks == g_gmasks).all(), (cap, np.flatnonzero(gmasks != g_gmasks)[:10])
            assert (gchunks == g_gchunks).all(), (cap, np.flatnonzero((gchunks != g_gchunks).reshape(n, -1).any(axis=1))[:10])
            assert (gmasks[ng:] == 0).all() and (gchunks[ng:] == 0).all()
            for first in GW.RECOVERING.get((name, cap), ()):
                g = int(want[first])
                mem = CM.members(want, g)
                assert mem[0] == first and (mem[0] // 64) < (mem[-1] // 64)
                assert gmasks[g] == geo.FULL_MASK, (cap, g, hex(int(gmasks[g])))
                assert (gchunks[g].reshape(-1) == payload[frame[first]]).all()
                assert (masks[mem] != geo.FULL_MASK).all()
        finally:
            auto.close()
            given.close()


# ------------------------------------------------------------------------------------------------ 2. automatic grouping, capture path
def test_automatic_grouping_across_steps_capture_path(CAPTURED):
    uniq, idx = CAPTURED
    raw = uniq[idx]
    n = len(raw)
    usable = GW.capture_usable()
    kw = dict(size=GW.CAPTURE_SIZE, fmt=FMT)
    plain = D.HipDecoder(0, MODE)
    try:
        _, rchunks, rmasks, rstatus = plain.scan_extract_decode_batch(raw, **kw)
        rccm = plain.get_ccm()
    finally:
        plain.close()
    assert ((rstatus > 0) == usable).all(), np.flatnonzero((rstatus > 0) != usable)
    for cap in GW.CAPTURE_CAPS:
        auto, given = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
        try:
            ng, chunks, masks, status, groups, gchunks, gmasks = auto.scan_extract_decode_batch_combined(raw, min_agree_permille=AGREE, max_group=cap, **kw)
            sym, col = auto.tap(D.TAP_SYMBOLS, n), auto.tap(D.TAP_COLORS, n)
            want = CM.group_captures(sym, col, usable=status > 0, min_agree_permille=AGREE, max_group=cap)
            assert want.tolist() == _synthetic_groups("straddle", cap, usable).tolist(), cap
            assert groups.tolist() == want.tolist(), (cap, np.flatnonzero(groups != want)[:10])
            assert ng == CM.n_groups(want)
            assert (status == rstatus).all() and (chunks == rchunks).all() and (masks == rmasks).all() and _same_ccm(auto.get_ccm(), rccm)
            g_ng, _, _, _, g_groups, g_gchunks, g_gmasks = given.scan_extract_decode_batch_combined(raw, groups=want, max_group=cap, **kw)
            assert g_ng == ng and g_groups.tolist() == want.tolist()
            assert (gmasks == g_gmasks).all() and (gchunks == g_gchunks).all()
            assert (gmasks[ng:] == 0).all() and (gchunks[ng:] == 0).all()
        finally:
            auto.close()
            given.close()


# ------------------------------------------------------------------------------------------------ 3. the stream calls, rendered frames
def _calls(sizes):
    """[(lo, n, flush)]: the last call and a call without captures are flushed"""
    out, lo = [], 0
    for i, n in enumerate(sizes):
        out.append((lo, n, i == len(sizes) - 1 or n == 0))
        lo += n
    return out


def _check_sequence(res, taps, usable, cap, name, ref, n_total):
    """res[c] = (n_closed, chunks, masks, groups, gchunks, gmasks, gsizes) of call c; taps[c] = its (symbols, colours); ref = the plain combined
    call on the whole batch: (ng, chunks, masks, groups, gchunks, gmasks)"""
    model, vetted = SM.StreamModel(AGREE, cap), SM.StreamModel(AGREE, cap)
    ssym, scol = GW.synthetic_cells(GW.RUN_LISTS[name])
    lo = 0
    for c, r in enumerate(res):
        n = len(r[1])
        _check_call_shape(r, n)
        u = usable[lo:lo + n]
        flush = c == len(res) - 1 or n == 0
        out, closed, gsizes = model.call(taps[c][0], taps[c][1], u, flush=flush)
        v_out, _, v_sizes = vetted.call(ssym[lo:lo + n], scol[lo:lo + n], u, flush=flush)
        assert out.tolist() == v_out.tolist() and gsizes == v_sizes, c                   # the batch behaves as the CPU test vetted it
        assert r[3].tolist() == out.tolist(), (c, np.flatnonzero(r[3] != out)[:10])
        assert r[0] == len(closed) and r[6][:r[0]].tolist() == gsizes, (c, r[0], len(closed))
        lo += n
    assert lo == n_total
    ng, chunks, masks, groups, gchunks, gmasks = ref
    gsizes, smasks, schunks = _closed(res)
    assert sum(r[0] for r in res) == ng
    assert gsizes.tolist() == np.bincount(groups[groups >= 0], minlength=ng).tolist()
    assert (smasks == gmasks[:ng]).all(), np.flatnonzero(smasks != gmasks[:ng])[:10]
    assert (schunks == gchunks[:ng]).all()
    assert (np.concatenate([r[1] for r in res]) == chunks).all() and (np.concatenate([r[2] for r in res]) == masks).all()


@pytest.mark.parametrize("case", GW.STREAM_CASES, ids=lambda c: f"{c[0]}-{c[1]}-" + "x".join(map(str, c[2])))
def test_stream_walk_across_steps(RENDERED, case):
    name, cap, sizes = case
    batch = _batch(RENDERED, name)
    n_total = len(batch)
    one, dec = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        ref = one.decode_batch_combined(batch, min_agree_permille=AGREE, max_group=cap)
        rccm = one.get_ccm()
        res, taps = [], []
        for lo, n, flush in _calls(sizes):
            res.append(dec.decode_batch_combined_stream(batch[lo:lo + n] if n else None, flush=flush, min_agree_permille=AGREE, max_group=cap))
            taps.append((dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)) if n else (np.zeros((0, 1), np.uint8),) * 2)
        ccm = dec.get_ccm()
    finally:
        one.close()
        dec.close()
    _check_sequence(res, taps, np.ones(n_total, bool), cap, name, ref, n_total)
    assert _same_ccm(ccm, rccm)


# ------------------------------------------------------------------------------------------------ 4. the stream calls, capture path
@pytest.mark.parametrize("case", GW.STREAM_CAPTURE_CASES, ids=lambda c: f"{c[0]}-{c[1]}-" + "x".join(map(str, c[2])))
def test_stream_walk_across_steps_capture_path(CAPTURED, case):
    name, cap, sizes = case
    assert GW.RUN_LISTS[name] is GW.CAPTURE_RUNS
    uniq, idx = CAPTURED
    raw = uniq[idx]
    n_total = len(raw)
    kw = dict(size=GW.CAPTURE_SIZE, fmt=FMT)
    one, dec = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    try:
        ng, chunks, masks, status, groups, gchunks, gmasks = one.scan_extract_decode_batch_combined(raw, min_agree_permille=AGREE, max_group=cap, **kw)
        rccm = one.get_ccm()
        assert ((status > 0) == GW.capture_usable()).all()
        res, taps, stats = [], [], []
        for lo, n, flush in _calls(sizes):
            r = dec.scan_extract_decode_batch_combined_stream(raw[lo:lo + n] if n else None, flush=flush, min_agree_permille=AGREE, max_group=cap, **kw)
            stats.append(r[3])
            res.append(r[:3] + r[4:])
            taps.append((dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n)) if n else (np.zeros((0, 1), np.uint8),) * 2)
        ccm = dec.get_ccm()
    finally:
        one.close()
        dec.close()
    got_status = np.concatenate(stats)
    assert (got_status == status).all()
    _check_sequence(res, taps, got_status > 0, cap, name, (ng, chunks, masks, groups, gchunks, gmasks), n_total)
    assert _same_ccm(ccm, rccm)
