"""CPU: the symbol erasure retry's model (tests/symbol_erasure_model.py) on the case set of tests/symbol_erasure_cases.py, fed by the oracle alone:
pyref.oracle_decode for the mask and chunks without the retry, pyref.oracle_stage for symbols and positions, co_threshold_bitplane for the plane.

- Bit order: on clean frames of each mode the hash the model reads at the oracle's positions equals the decoded symbol's tile on all 36 interior
  bits of every cell. (The 28 border bits of a cell see the neighbouring cells through the 5x5 threshold window: about one clean cell in a
  hundred is 2 or 4 bits from its tile there. The test bounds that at 4 and at 3 % of the cells, so the thresholds the tests use, 6 and 5, are
  never reached by a clean cell.)
- Promise: every chunk the model adds equals the payload, nothing else changes, and each construction promise of the case set holds in the
  model's record (order, ties at the cap, nothing flagged, status 1 refused by the slack, two nibbles, all blocks but one, several missing
  chunks, one round of four concurrently retried blocks, all delivered, non-zero drift on damaged cells, exact distances t_sym - 1 and t_sym on deciding bytes).
- Sensitivity: every switch of the model (MUTANTS, GROUP_MUTANTS) changes (mask, chunks) on at least one frame / group of every mode's set at
  t_sym = 6 and the default cap.
- The pieces the model puts together equal colour_erasure_model.retry_block on every block it retried.

Time (measured): the pure-Python Reed-Solomon model takes about 2 ms per block; the specified model over one mode's frames makes 69 / 41 / 55
decodes in 0.14 / 0.09 / 0.10 s (modes 68 / 67 / 66), and with symbol_erasure_model's per-(block, erasures) cache the 20 frame mutants and 5 group
mutants add only the blocks they decide differently: every test here runs in under 9 s, most of it the oracle and combine_cells.
"""
import time

import numpy as np
import pytest

from libcimbar_amd import geometry, modeb
from tests import colour_erasure_model as CE
from tests import combine_model as CM
from tests import symbol_erasure_cases as K
from tests import symbol_erasure_model as M


def _sym_chunks(geo):
    return geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)


@pytest.mark.parametrize("mode", K.MODES)
def test_bit_order_on_clean_frames(mode):
    geo = geometry.for_mode(mode)
    payload = K.framegen.synth_payload(3, seed=77 + mode, mode=mode)
    frames = K.framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy()
    grid = geo.cell_positions().astype(np.int64)
    interior = np.uint64(int("".join("0" if r in (0, 7) or c in (0, 7) else "1" for r in range(8) for c in range(8)), 2))
    tiles = np.asarray(modeb.TILE_HASHES, np.uint64)
    for r in K.oracle_run(mode, frames):
        assert r["mask"] == geo.FULL_MASK and (r["positions"] == grid).all()
        h = CM.cell_hashes(mode, r["plane"], r["positions"] - grid, True)
        assert (((h ^ tiles[r["symbols"] & 15]) & interior) == 0).all(), "an interior bit of a clean cell differs from its tile"
        d = M.cell_distances(mode, r["plane"], r["symbols"], r["positions"], True, absolute=True)
        assert (d == CM._popcount64(h ^ tiles[r["symbols"] & 15])).all()
        assert d.max() <= 4 and (d > 0).mean() < 0.03, (int(d.max()), float((d > 0).mean()))
        # the same through the drift form of the argument, flooded or not
        assert (M.cell_distances(mode, r["plane"], r["symbols"], np.zeros((geo.NCELLS, 2), np.int8), False) == d).all()


@pytest.mark.parametrize("mode", K.MODES)
def test_promises(mode):
    geo = geometry.for_mode(mode)
    cs, runs = K.case_set(mode), K.oracle_frames(mode)
    p, n, bpc = geo.RS_PARITY, geo.RS_BLOCK, geo.CHUNK // geo.RS_DATA
    E, symc = p - 8, _sym_chunks(geo)
    grid = geo.cell_positions().astype(np.int64)
    t0 = time.time()
    before = len(M._rs_cache)
    res = K.model_frames(mode, runs)
    spent, decodes = time.time() - t0, len(M._rs_cache) - before
    print(f"mode {mode}: {decodes} Reed-Solomon model decodes in {spent:.2f} s")
    for f, (m1, c1, rec, d) in enumerate(res):
        r = runs[f]
        pay = cs["payload"][f].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
        assert m1 & r["mask"] == r["mask"] and (m1 ^ r["mask"]) >> symc == 0
        for j in range(geo.CHUNKS_PER_FRAME):
            if (r["mask"] >> j) & 1 or j >= symc:
                assert (c1[j] == r["chunks"][j]).all()
            elif (m1 >> j) & 1:
                assert (c1[j] == pay[j]).all(), (f, j)
            else:
                assert not c1[j].any(), (f, j)
        # the pieces equal the colour retry's retry_block
        for b, rb in enumerate(rec or []):
            if rb["status"] != 2:
                st, _, er = CE.retry_block(M.stream_bytes(geo, r["symbols"])[b], rb["scores"], rb["ok"], p, E)
                assert (st, er) == (rb["status"], rb["erasures"]), (f, b)
    # frame 0: all delivered, the retry returns at once
    assert runs[0]["mask"] == geo.FULL_MASK and res[0][2] is None
    # frame 1: several missing chunks (every wavefront has blocks to retry), all won back
    m1, c1, rec, d = res[1]
    mk = cs["marks"][1]
    assert bin(~runs[1]["mask"] & ((1 << symc) - 1)).count("1") >= 4 and m1 == geo.FULL_MASK
    pairs = M._stream_pairs(geo, d).reshape(geo.SYM_BLOCKS, n, 2)
    blocks = M.stream_bytes(geo, runs[1]["symbols"])

    def outcome(b, **kw):
        rules = M.rules_with(**kw)
        sc = M.byte_scores(geo, d, K.T_SYM, rules)[b]
        er = M._select(sc, E + rules["cap"], rules)
        return M._retry_block(blocks[b], er, False, p, rules)[0]

    o = rec[mk["order"]]                                 # more flagged bytes than the cap; the order decides
    assert int((o["scores"] > 0).sum()) > E and len(o["erasures"]) == E and o["status"] == 1 and outcome(mk["order"], order="lowest") != 1
    t = rec[mk["ties"]]                                  # a tie across the cap
    ranked = M._select(t["scores"], n, M.RULES)
    assert len(ranked) > E and t["scores"][ranked[E - 1]] == t["scores"][ranked[E]] and t["status"] == 1 and outcome(mk["ties"], ties="higher") != 1
    c = rec[mk["cap"]]
    assert c["status"] == 1 and outcome(mk["cap"], cap=1) != 1 and outcome(mk["cap"], cap=-1) != 1
    k = rec[mk["okblock"]]                               # errors-only decoding accepted it: no erasure although a byte is flagged
    assert k["ok"] and k["erasures"] == [] and (k["scores"] > 0).any() and k["status"] == 1
    x = rec[mk["exact"]]                                 # distances exactly t_sym and t_sym - 1 on bytes that decide the block; two nibbles
    px = pairs[mk["exact"]]
    assert x["status"] == 1 and any(px[kk].max() == K.T_SYM for kk in x["erasures"]) and (px.max(1) == K.T_SYM - 1).any()
    assert outcome(mk["exact"], bias=1) != 1 and outcome(mk["exact"], bias=-1) != 1
    assert any(px[kk, 0] < K.T_SYM <= px[kk, 1] for kk in x["erasures"]) and outcome(mk["exact"], nibble="first") != 1
    # frame 4: one round of the four wavefronts, blocks 4 .. 7: each failed errors-only decoding, is retried with erasures of its own and is
    # accepted -- and with the score row or the erasure list of any other block of the round it is not
    m4, c4, rec4, d4 = res[4]
    rnd = sorted(cs["marks"][4].values())
    assert rnd == [4, 5, 6, 7] and m4 == geo.FULL_MASK
    b4, sc4 = M.stream_bytes(geo, runs[4]["symbols"]), M.byte_scores(geo, d4, K.T_SYM)
    for b in rnd:
        assert not rec4[b]["ok"] and rec4[b]["erasures"] and rec4[b]["status"] == 1, b
        for o in rnd:
            if o != b:
                assert set(rec4[o]["erasures"]) != set(rec4[b]["erasures"])
                assert M._retry_block(b4[b], rec4[o]["erasures"], False, p, M.RULES)[0] != 1, (b, o)
                assert M._retry_block(b4[b], M._select(sc4[o], E, M.RULES), False, p, M.RULES)[0] != 1, (b, o)
    # frame 2: refused by the slack although libcorrect decodes it; nothing flagged; all blocks but one
    m2, c2, rec2, _ = res[2]
    mk2 = cs["marks"][2]
    b2 = M.stream_bytes(geo, runs[2]["symbols"])
    for name in ("slack", "slack5"):
        s = rec2[mk2[name]]
        assert s["status"] == 0 and M.rs_decode(b2[mk2[name]], s["erasures"], p)[0] == 1, name
    assert len(rec2[mk2["slack"]]["erasures"]) == E and len(rec2[mk2["slack5"]]["erasures"]) == E - 1
    bl = rec2[mk2["blind"]]
    assert bl["status"] == -2 and not bl["ok"] and not (bl["scores"] > 0).any()
    j = mk2["blind"] // bpc
    assert [rec2[j * bpc + q]["status"] for q in range(bpc)].count(1) == bpc - 1 and not (m2 >> j) & 1 and not c2[j].any()
    # frame 3: the shifted copy of frame 1: the damaged cells have drifted, the result is frame 1's
    damaged = res[3][3] >= K.T_SYM
    assert damaged.sum() > 50 and ((runs[3]["positions"] - grid)[damaged] != 0).any(1).all()
    assert res[3][0] == m1 and (res[3][1][:symc] == c1[:symc]).all()


def _differs(a, b):
    return any(x[0] != y[0] or (x[1] != y[1]).any() for x, y in zip(a, b))


@pytest.mark.parametrize("mode", K.MODES)
def test_every_rule_is_seen_by_the_frames(mode):
    runs = K.oracle_frames(mode)
    spec = K.model_frames(mode, runs)
    survivors = [mu for mu in M.MUTANTS if not _differs(spec, K.model_frames(mode, runs, rules=M.rules_with(**{mu[0]: mu[1]})))]
    assert not survivors, f"mode {mode}: the case set does not see {survivors}"


def group_results(mode, rules=None):
    """-> per group (gmask, gchunks, record, members' model results), from the oracle alone. The retry-off group result is put together here:
    the combined decode's symbol chunks (combined_symbol_mask; its bytes are the errors-only messages), else the lowest member's; the
    colour chunks from the members."""
    geo = geometry.for_mode(mode)
    cs, runs = K.case_set(mode), K.oracle_group_caps(mode)
    rules = M.RULES if rules is None else rules
    on = K.model_frames(mode, runs)                      # (the members' own retry is the specified one: the switch under test is the group's)
    bpc = geo.CHUNK // geo.RS_DATA
    out = []
    for g in range(int(cs["groups"].max()) + 1):
        mem = CM.members(cs["groups"], g)
        cells, margins, disputed = K.combine_inputs(mode, runs, mem)
        blocks = M.stream_bytes(geo, cells & 15)
        cmask, _ = M.combined_symbol_mask(geo, blocks) if disputed else (0, None)
        g0 = np.zeros((geo.CHUNKS_PER_FRAME, geo.CHUNK), np.uint8)
        m0 = 0
        for j in range(geo.CHUNKS_PER_FRAME):
            if (cmask >> j) & 1:
                g0[j] = np.concatenate([M.rs_decode(blocks[j * bpc + q], [], geo.RS_PARITY)[1] for q in range(bpc)])
                m0 |= 1 << j
                continue
            for c in mem:
                if (runs[c]["mask"] >> j) & 1:
                    g0[j], m0 = runs[c]["chunks"][j], m0 | (1 << j)
                    break
        gm, gc, rec = M.retry_group(geo, cells, margins, m0, g0, [on[c][0] for c in mem], [on[c][1] for c in mem], disputed=disputed, rules=rules)
        out.append((gm, gc, rec, m0))
    return out


@pytest.mark.parametrize("mode", K.MODES)
def test_groups_promise_and_sensitivity(mode):
    geo = geometry.for_mode(mode)
    cs = K.case_set(mode)
    symc = _sym_chunks(geo)
    spec = group_results(mode)
    for g, (gm, gc, rec, m0) in enumerate(spec):
        pay = cs["group_payload"][g].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
        assert gm & m0 == m0
        for j in range(symc):
            assert (gc[j] == pay[j]).all() if (gm >> j) & 1 else not gc[j].any(), (g, j)
    # the constructed pair: chunks 0 and 1 are won by the group retry alone, with more disputed bytes than the cap in chunk 0
    gm, gc, rec, m0 = spec[0]
    assert m0 & 3 == 0 and gm & 3 == 3
    r0 = rec[0]
    assert int((r0["scores"] != M.MARGIN_NONE).sum()) > geo.RS_PARITY - 8 and len(set(r0["scores"].tolist())) >= 3
    print(f"mode {mode}: group masks without / with the retry", [(hex(s[3]), hex(s[0])) for s in spec])
    survivors = [mu for mu in M.GROUP_MUTANTS if not _differs(spec, group_results(mode, M.rules_with(**{mu[0]: mu[1]})))]
    assert not survivors, f"mode {mode}: the group set does not see {survivors}"
