"""CPU: the colour erasure retry's model (tests/colour_erasure_model.py) against the classifier restatement and the oracle.

- Margin: for every palette colour, grey / white / black and 2^20 stratified RGB values, with and without a matrix, the model's margin equals
  colour_cases.tie_margin and its class colour_cases.best_color; pure green, cyan and yellow have 510 * 255 = 130 050, pure magenta 510 * 765 = 390 150 (it is the
  only colour whose relative colour has no neighbour 255 away), grey / white / black 0; for the
  four-colour palette the margin equals 510 * (best - second-best of the four terms the device ranks).
- Selection: ties go to the lower position, the cap holds, a failed block with no flagged byte is not retried, the slack rule rejects a
  decode that uses up the parity.
- Threshold: the one value the tests use flags no cell of the clean rendered frames, in any mode.
- Glare: on the glare set run through the oracle for colours, positions, matrix and masks, the model delivers strictly more colour chunks
  than the oracle alone in every mode, every chunk it adds equals the payload, and nothing else changes.
"""
import numpy as np
import pytest

from libcimbar_amd import geometry
from oracle import pyref
from tests import colour_cases as C
from tests import colour_erasure_cases as K
from tests import colour_erasure_model as M
from tests import rs_cases


def _ccm10(ccm):
    return np.array(list(ccm.m) + [ccm.active], np.float32)


def _four_term_margin(rgb, m):
    """510 * (largest - second-largest) of the four terms green, cyan, yellow, magenta (k4_frame.hip.inc's shortcut)"""
    c0, c1, c2 = C._fixed(*C._transformed(rgb, m))
    r0, r1, r2 = c0 - c1, c1 - c2, c2 - c0
    t = np.sort(np.stack([r1 - r0, r2 - r0, r1 - r2, r0 - r1], 1), 1)
    return 510 * (t[:, 3] - t[:, 2])


MATRICES = [None, np.array([1.1, -0.08, 0.02, -0.05, 0.93, 0.07, 0.03, -0.11, 1.21], np.float32),
            np.array([0.6, 0.3, 0.1, 0.2, 0.7, 0.1, 0.1, 0.2, 0.9], np.float32)]


@pytest.mark.parametrize("mi", range(len(MATRICES)))
def test_margin_equals_tie_margin(mi):
    m = MATRICES[mi]
    ccm10 = np.concatenate([m if m is not None else np.zeros(9, np.float32), [1.0 if m is not None else 0.0]]).astype(np.float32)
    special = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [37, 37, 37]], np.float32)
    rgb = np.concatenate([C.PALETTE_B.astype(np.float32), special, C.stratified_rgb(20, seed=3)])
    got = M.margins(rgb, ccm10)
    assert (got == C.tie_margin(rgb, m, C.PALETTE_B)).all()
    assert (M.classes(rgb, ccm10) == C.best_color(rgb, m, C.PALETTE_B)).all()
    assert (got == _four_term_margin(rgb, m)).all()
    if m is None:
        assert got[:4].tolist() == [510 * 255] * 3 + [510 * 765] and (M.classes(rgb[:4], ccm10) == np.arange(4)).all()
        assert (got[4:8] == 0).all()
    # an inactive matrix is no matrix, whatever its nine numbers are
    off = ccm10.copy()
    off[9] = 0
    assert (M.margins(rgb[:4096], off) == C.tie_margin(rgb[:4096], None, C.PALETTE_B)).all()


def test_selection_rank_and_cap():
    s = np.zeros(155, np.int64)
    s[[9, 3, 50, 120, 7]] = [5, 5, 9, 1, -4]
    assert M.select(s, 30) == [50, 3, 9, 120]
    assert M.select(s, 2) == [50, 3]
    assert M.select(s, 0) == []
    assert M.select(np.full(155, 7), 22) == list(range(22))
    assert M.select(np.zeros(155, np.int64), 22) == []


def test_retry_block_rules():
    geo = geometry.for_mode(68)
    p, n = geo.RS_PARITY, geo.RS_BLOCK
    g = np.random.default_rng(5)
    word = rs_cases.encode(g.integers(0, 256, (1, n - p), dtype=np.uint8), p)[0]
    # 20 damaged bytes: errors-only decoding (15 at most) fails
    bad = g.choice(n, 20, replace=False)
    blk = word.copy()
    blk[bad] ^= g.integers(1, 256, 20).astype(np.uint8)
    assert not M.errors_only_ok(blk, p)
    none = np.zeros(n, np.int64)
    assert M.retry_block(blk, none, False, p, p - 8)[0] == -2                  # nothing flagged: not retried
    flagged = none.copy()
    flagged[bad] = 100
    st, msg, er = M.retry_block(blk, flagged, False, p, p - 8)
    assert st == 1 and sorted(er) == sorted(bad.tolist()) and (msg == word[:n - p]).all()
    # 15 of them flagged, 5 left as errors: 2 * 5 > 30 - 15 - 6 -- the slack rule turns the (correct) decode down
    part = none.copy()
    part[bad[:15]] = 100
    rc, m2, w2, in_pad = M.E.decode(blk, M.select(part, p - 8), p)
    assert M.E.status(rc, w2, in_pad, p) == 1 and M.locator_order(blk, M.select(part, p - 8), p) == 5
    assert M.retry_block(blk, part, False, p, p - 8)[0] == 0
    # a block errors-only decoding passed is decoded with no erasures, whatever is flagged
    few = word.copy()
    few[bad[:5]] ^= 1
    st, msg, er = M.retry_block(few, flagged, True, p, p - 8)
    assert st == 1 and er == [] and (msg == word[:n - p]).all()


@pytest.mark.parametrize("mode", K.MODES)
def test_threshold_flags_no_clean_cell(mode):
    geo = geometry.for_mode(mode)
    lowest = None
    for seed in (K.GLARE_SEED, 11, 31):
        fr, _ = K.frames(mode, 8, seed)
        ccm = None
        for f in range(len(fr)):
            _, _, mask, ccm = pyref.oracle_decode(fr[f], 0, 2, ccm, mode=mode)
            assert mask == geo.FULL_MASK
            _, col, pos = pyref.oracle_stage(mode=mode)
            mg = M.margins(M.cell_means(fr[f], pos), _ccm10(ccm))
            lowest = int(mg.min()) if lowest is None else min(lowest, int(mg.min()))
    print(f"mode {mode}: lowest margin of a clean rendered cell {lowest}, threshold {K.MARGIN}")
    assert lowest >= K.MARGIN


@pytest.mark.parametrize("mode", K.MODES)
def test_glare_model_recovers_more(mode):
    geo = geometry.for_mode(mode)
    fr, payload, kinds, _ = K.glare_set(mode)
    symc = K.sym_chunks(geo)
    ccm = None
    before = after = 0
    for f in range(len(fr)):
        _, chunks, mask, ccm = pyref.oracle_decode(fr[f], 0, 2, ccm, mode=mode)
        _, col, pos = pyref.oracle_stage(mode=mode)
        means = M.cell_means(fr[f], pos)
        assert (M.classes(means, _ccm10(ccm)) == col).all(), "the model's class differs from the oracle's colour"
        m1, c1, worked = M.retry_frame(geo, col, M.margins(means, _ccm10(ccm)), mask, chunks, K.MARGIN)
        assert worked == ((mask >> symc) != (geo.FULL_MASK >> symc))
        assert m1 & mask == mask and (m1 ^ mask) & ((1 << symc) - 1) == 0
        p = payload[f].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
        for j in range(geo.CHUNKS_PER_FRAME):
            if (mask >> j) & 1:
                assert (c1[j] == chunks[j]).all()
            if (m1 >> j) & 1:
                assert (c1[j] == p[j]).all(), (f, j, kinds[f])
            else:
                assert not c1[j].any()
        before += bin(mask >> symc).count("1")
        after += bin(m1 >> symc).count("1")
    print(f"mode {mode}: colour chunks delivered {before} -> {after} of {len(fr) * (geo.CHUNKS_PER_FRAME - symc)}")
    assert after > before
