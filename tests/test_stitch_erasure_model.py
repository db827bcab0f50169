"""CPU: the case set of tests/stitch_erasure_cases.py against tests/stitch_erasure_model.py fed by the oracle, modes 68 / 67 / 66. These are
conditions on the inputs; the GPU tests (tests/test_gpu_stitch_erasure.py) rely on them.

- lay-out: the slots each batch promises (B's, Cd's, the complete one, the ones of no candidate) are what the stitch model and an errors-only
  decode of its cells make of the oracle's per-capture cells; on the target case every failing symbol block of B has flagged cells from both
  captures, on the axis-0 "across" cases some failing block's flagged cells all come from one capture.
- sensitivity, on the target case: with the retry off B's slot lacks symbol chunks and a colour chunk; with it on the mask is full and the
  chunks are B's payload; each retry alone delivers its own kind only; every mutant of symbol_erasure_model.MUTANTS that bears on distance or
  selection changes the result, and so does the "wrong source" mutant, which takes every confidence from capture k.
- every case: the mask with the retry on is a superset of the mask with it off, chunks already delivered are untouched, and no slot -- the
  wrong-direction ones included -- holds a chunk that is not the payload of a frame shown.
"""
import functools

import numpy as np
import pytest

from libcimbar_amd import geometry
from tests import colour_erasure_model as CE
from tests import erasure_model as E
from tests import stitch_erasure_cases as S
from tests import stitch_erasure_model as SE
from tests import stitch_model as SM
from tests import symbol_erasure_cases as K
from tests import symbol_erasure_model as M

# the mutants of the symbol retry that change a distance or the selection (the others concern acceptance and the chunk rule, which the stitched
# retry takes from er_retry_blocks unchanged; "position" needs a capture that took the flood pass, which these rendered captures do not)
DIST_SELECT_MUTANTS = [m for m in M.MUTANTS if m[0] in ("window", "pairing", "bias", "nibble", "order", "ties", "cap")]


def errors_only_slot(geo, cells):
    """the stitched decode of one slot's cells without any retry: -> (mask, chunks (CHUNKS, CHUNK)). One aligner state over the symbol blocks,
    then the colour blocks: a chunk is delivered when all its blocks decoded and the last block of the chunk before it did."""
    blocks = np.concatenate([M.stream_bytes(geo, cells & 15), CE.stream_bytes(geo, cells >> 4)])
    bpc = geo.CHUNK // geo.RS_DATA
    out = np.zeros((geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    mask, carried = 0, False
    for j in range(geo.CHUNKS_PER_FRAME):
        res = [E.decode(blocks[j * bpc + q], [], geo.RS_PARITY) for q in range(bpc)]
        ok = [r[0] >= 0 for r in res]
        if all(ok) and not carried:
            mask |= 1 << j
            out[j] = np.concatenate([np.asarray(r[1], np.uint8)[:geo.RS_DATA] for r in res])
        carried = not ok[-1]
    return mask, out


@functools.lru_cache(maxsize=None)
def oracle_case(mode, case):
    geo = geometry.for_mode(mode)
    caps, shown, where = S.batch(mode, case)
    runs = K.oracle_run(mode, caps)
    tears, _, cells = SM.stitch_batch(mode, [r["symbols"] for r in runs], [r["colours"] for r in runs], case[1])
    margs = [CE.margins(CE.cell_means(caps[k], r["positions"]), r["ccm"]) for k, r in enumerate(runs)]
    slots = 2 * len(tears)
    m0, c0 = np.zeros(slots, np.uint32), np.zeros((slots, geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
    for g in range(slots):
        if tears[g // 2, 0] >= 0:
            m0[g], c0[g] = errors_only_slot(geo, cells[g])
    return dict(runs=runs, tears=tears, cells=cells, margs=margs, m0=m0, c0=c0, shown=shown, where=where)


def _distances(mode, oc, rules=M.RULES):
    return [M.cell_distances(mode, r["plane"], r["symbols"], r["positions"], True, rules, absolute=True) for r in oc["runs"]]


def _on(mode, case, t_sym=S.T_SYM, colour_margin=S.MARGIN, rules=M.RULES, wrong=None):
    oc = oracle_case(mode, case)
    return SE.retry_batch(mode, case[1], oc["tears"], oc["cells"], _distances(mode, oc, rules), oc["margs"], oc["m0"], oc["c0"], wrong=wrong,
                          t_sym=t_sym, colour_margin=colour_margin, rules=rules)


def _symc(geo):
    return geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)


@pytest.mark.parametrize("mode", S.MODES)
def test_target_case_is_sensitive(mode):
    geo = geometry.for_mode(mode)
    case = S.TARGET
    oc = oracle_case(mode, case)
    b = oc["where"]["b"]
    payB = S.frames_of(mode)["pay"]["B"].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
    sym_mask = (1 << _symc(geo)) - 1
    m0 = int(oc["m0"][b])
    assert m0 & 0xF == 0 and m0 & sym_mask != sym_mask, hex(m0)                    # the four designed symbol chunks are missing ...
    assert (m0 | sym_mask) != geo.FULL_MASK, hex(m0)                              # ... and so is a colour chunk
    m1, c1, d1, g1 = _on(mode, case)
    assert int(m1[b]) == geo.FULL_MASK and (c1[b] == payB).all(), hex(int(m1[b]))
    assert (d1[b] != SE.DIST_SKIPPED).any() and (g1[b] != SE.MARGIN_SKIPPED).any()
    # every repainted byte has a cell under the suggested margin (which flags the byte), taken in the capture the cell came from
    src = SE.source(mode, case[1], oc["tears"][b // 2])[b % 2]
    il = geo.interleave_indices()
    cb, pos = S.frames_of(mode)["colour_block"], S.frames_of(mode)["pos_b"]
    cells = np.array([il[(geo.RS_BLOCK * cb + k) * 4 + q] for k in pos for q in range(4)])
    assert (g1[b][cells].reshape(-1, 4).min(1) < S.MARGIN).all()
    assert len(set(src[cells].tolist())) == 2, "the repainted cells come from one capture only"
    # each retry alone
    ms, cs, _, gs = _on(mode, case, colour_margin=0)
    assert int(ms[b]) == m0 | sym_mask and (gs == SE.MARGIN_SKIPPED).all()
    mc, cc, dc, _ = _on(mode, case, t_sym=0)
    assert int(mc[b]) == m0 | (geo.FULL_MASK & ~sym_mask) and (dc == SE.DIST_SKIPPED).all()
    # every failing symbol block has flagged cells from both captures
    dist = SE.by_source(src, *_distances(mode, oc)[b // 2:b // 2 + 2])
    flagged = dist - S.T_SYM + 1 > 0
    for name, blk in K.case_set(mode)["marks"][1].items():
        if name == "okblock":
            continue
        bc = il[geo.RS_BLOCK * blk * 2:geo.RS_BLOCK * (blk + 1) * 2]
        assert len(set(src[bc][flagged[bc]].tolist())) == 2, name
    # the mutants
    for key, val in DIST_SELECT_MUTANTS:
        mm, cm, _, _ = _on(mode, case, rules=M.rules_with(**{key: val}))
        assert int(mm[b]) != int(m1[b]) or (cm[b] != c1[b]).any(), (key, val)
    mw, cw, _, _ = _on(mode, case, wrong="k")
    assert int(mw[b]) != int(m1[b]) or (cw[b] != c1[b]).any(), "every confidence from capture k: no difference"


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
@pytest.mark.parametrize("mode", S.MODES)
def test_layout_superset_and_genuine_chunks(mode, case):
    geo = geometry.for_mode(mode)
    oc = oracle_case(mode, case)
    where, m0, c0 = oc["where"], oc["m0"], oc["c0"]
    sym_mask = (1 << _symc(geo)) - 1
    live = np.repeat(oc["tears"][:, 0] >= 0, 2)
    assert live[where["b"]] and int(m0[where["b"]]) & sym_mask != sym_mask
    assert not live[list(where["dead"])].any()
    if where["cd"] is not None:
        assert where["cd"] > 3 and live[where["cd"]]
        assert int(m0[where["cd"]]) & sym_mask == sym_mask and int(m0[where["cd"]]) != geo.FULL_MASK      # the colour retry only
        assert live[where["complete"]] and int(m0[where["complete"]]) == geo.FULL_MASK
    else:
        assert where["b"] > 3
    if case[0] == "across" and case[1] == 0:
        # the split lies near the boundary of the interleave's two partitions: some failing block's flagged cells all come from one capture
        src = SE.source(mode, 0, oc["tears"][where["b"] // 2])[where["b"] % 2]
        il = geo.interleave_indices()
        k = where["b"] // 2
        flagged = SE.by_source(src, *_distances(mode, oc)[k:k + 2]) - S.T_SYM + 1 > 0
        sides = {name: set(src[bc][flagged[bc]].tolist()) for name, blk in K.case_set(mode)["marks"][1].items()
                 for bc in [il[geo.RS_BLOCK * blk * 2:geo.RS_BLOCK * (blk + 1) * 2]]}
        assert any(len(v) == 1 for v in sides.values()), sides
    m1, c1, _, _ = _on(mode, case)
    pay = S.frames_of(mode)["pay"]
    for g in range(len(m0)):
        assert int(m0[g]) & ~int(m1[g]) == 0, (g, hex(int(m0[g])), hex(int(m1[g])))
        for j in range(geo.CHUNKS_PER_FRAME):
            if (int(m0[g]) >> j) & 1:
                assert (c1[g, j] == c0[g, j]).all(), (g, j)
    assert int(m1[where["b"]]) == geo.FULL_MASK and (c1[where["b"]].reshape(-1) == pay["B"]).all()
    if where["cd"] is not None:
        assert int(m1[where["cd"]]) == geo.FULL_MASK and (c1[where["cd"]].reshape(-1) == pay["Cd"]).all()
    assert not m1[~live].any() and not c1[~live].any()
    bad = S.genuine(mode, oc["shown"], m1, c1)
    assert bad is None, bad
