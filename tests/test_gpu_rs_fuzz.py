"""GPU: Reed-Solomon decode fuzzed through the whole pipeline, in every mode k_rs is built for (68, 67, 66 and the legacy 4 and 8). Frames are
rendered from hand-made streams of RS blocks (valid codewords of the mode's RS(n, n - p) with injected byte errors: 0 .. t + 7 per block at random,
plus the edge families of tests/rs_cases.py: exactly t-1 .. t+2 errors at the lane-register and message/parity boundaries, zero bytes, errors in the
shortened code's padding, vanishing leading syndromes), so every block of a frame exercises K3 with a known error pattern; per-block outcome and
bytes are compared with the oracle's literal libcorrect restatement -- including the > t error regime where libcorrect may "succeed" with wrong
data -- and, where the reference build is present, with libcorrect itself."""
import functools

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen
from oracle import pyref
from oracle.pyref import P
from tests import rs_cases
from tests.test_gpu_modes import check

pytestmark = pytest.mark.gpu

MODES = [68, 67, 66, 4, 8]
# frames of hand-made blocks per mode (mode 68: the 12 frames of 0..22 errors this test always had, then the widened set); 9 in mode 8: its
# 70 blocks are not a multiple of k_rs's 4 blocks per workgroup, so workgroups span two frames and the batch ends on a partial one
NFRAMES = {68: 4, 67: 16, 66: 16, 4: 9, 8: 9}


@pytest.fixture(scope="module", params=MODES)
def MODE(request):
    return request.param


@pytest.fixture(scope="module")
def dec(MODE):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = D.HipDecoder(0, MODE)
    yield d
    d.close()


def _mode68_original_blocks():
    """the 12 frames (720 blocks of RS(155,125), 0..22 errors, a quarter each at random / front / tail / boundary positions) of seed 99"""
    g = np.random.default_rng(99)
    nframes = 12
    msgs = g.integers(0, 256, (nframes * 60, 125), dtype=np.uint8)
    blocks = framegen.rs_encode(torch.from_numpy(msgs)).numpy().copy()
    cases = []
    for b in range(blocks.shape[0]):
        ne = int(g.integers(0, 23))
        mode = b % 4
        if mode == 0:
            pos = g.choice(155, ne, replace=False)
        elif mode == 1:   # burst at the front
            pos = np.arange(ne)
        elif mode == 2:   # burst over the parity tail, including the very last byte (error location 0)
            pos = 154 - np.arange(ne)
        else:             # message/parity boundary
            pos = (118 + np.arange(ne)) % 155
        blocks[b, pos] ^= g.integers(1, 256, ne, dtype=np.uint8)
        cases.append((blocks[b].copy(), "random", msgs[b].copy() if ne <= 15 else None))
    return cases


@functools.lru_cache(maxsize=None)
def fuzz_set(mode):
    """(synth, cases in stream order, blocks (F, BLOCKS, n), frames (F, H, W, 3)): the mode's edge cases and random blocks, shuffled over the
    frames (so that they land in both streams and in every slot of a k_rs workgroup)"""
    synth = framegen.FrameSynth("cpu", mode)
    geo = synth.geo
    n, p = geo.RS_BLOCK, geo.RS_PARITY
    g = np.random.default_rng(4000 + mode)
    cases = rs_cases.edge_cases(g, n, p)
    total = NFRAMES[mode] * geo.BLOCKS
    cases += rs_cases.random_cases(g, n, p, total - len(cases), p // 2 + 7)
    cases = [cases[i] for i in g.permutation(len(cases))]
    if mode == 68:
        cases = _mode68_original_blocks() + cases
    nf = len(cases) // geo.BLOCKS
    blocks = np.stack([c[0] for c in cases]).reshape(nf, geo.BLOCKS, n)
    frames = synth.render(rs_cases.blocks_to_tiles(synth, blocks)).numpy()
    return synth, cases, blocks, frames


def _rs(L, block, n, parity):
    out = np.zeros(n - parity, np.uint8)
    return L.co_rs_decode(P(np.ascontiguousarray(block)), n, parity, P(out)), out


def _ref_rs(block, n, parity):
    R = pyref.ref_lib()
    if R is None:
        return None, None
    out = np.zeros(n - parity, np.uint8)
    return R.ref_rs_decode(P(np.ascontiguousarray(block)), n, parity, P(out)), out


def test_rs_blocks_with_known_error_patterns(dec, MODE):
    synth, cases, blocks, frames = fuzz_set(MODE)
    geo = synth.geo
    n, p, k, B, BPC = geo.RS_BLOCK, geo.RS_PARITY, geo.RS_DATA, geo.BLOCKS, geo.BLOCKS // geo.CHUNKS_PER_FRAME
    nframes = frames.shape[0]
    O = pyref.oracle_lib(MODE)

    dec.reset_ccm()
    # colour correction off: the colour stream must reach RS exactly as rendered, whatever the (garbage) headers say
    total, chunks, masks = dec.decode_batch(frames, color_correction=0)
    rs_ok = dec.tap(D.TAP_RS_OK, nframes)
    sym = dec.tap(D.TAP_SYMBOLS, nframes)
    col = dec.tap(D.TAP_COLORS, nframes)
    want_tiles = rs_cases.blocks_to_tiles(synth, blocks).numpy()
    assert (col.astype(np.int64) * 16 + sym == want_tiles).all(), "cells must reach RS exactly as rendered"

    ref_there = pyref.ref_lib() is not None
    regimes = dict(corrected=0, failed=0, padding=0, vanishing=0)
    want_plain = np.zeros((nframes, B, k), np.uint8)
    for f in range(nframes):
        for b in range(B):
            case = cases[f * B + b]
            rr, out = _rs(O, blocks[f, b], n, p)
            tag = f"mode {MODE} frame {f} block {b} ({case[1]})"
            assert bool(rs_ok[f, b]) == (rr > 0), f"{tag}: ok flag {rs_ok[f, b]} vs libcorrect restatement {rr}"
            rs_cases.check_promise(case, p, rr, out)
            if ref_there:
                r1, o1 = _ref_rs(blocks[f, b], n, p)
                assert bool(rs_ok[f, b]) == (r1 > 0) and (r1 <= 0 or (o1 == out).all()), f"{tag}: libcorrect {r1}"
            if rr > 0:
                want_plain[f, b] = out
                regimes["corrected"] += 1
                # a correction in the padding was dropped: the re-encoded message is then no codeword within t of the block
                if np.count_nonzero(rs_cases.encode(out[None], p)[0] != blocks[f, b]) > p // 2:
                    regimes["padding"] += 1
                c = b // BPC
                if masks[f] >> c & 1:      # the bytes of a delivered chunk (a dropped one is zeroed)
                    got = chunks[f, c, (b % BPC) * k:(b % BPC + 1) * k]
                    assert (got == out).all(), f"{tag}: bytes in chunk {c} differ from the libcorrect restatement's"
            else:
                regimes["failed"] += 1
            regimes["vanishing"] += case[1].startswith("vanishing")
    print(f"\nmode {MODE}: {nframes * B} blocks of RS({n},{k}): {regimes}")
    assert regimes["corrected"] and regimes["failed"] and regimes["padding"] and regimes["vanishing"]

    ccm = pyref.CoCcm()
    want_total = 0
    for f in range(nframes):
        r, want_chunks, want_mask, ccm = pyref.oracle_decode(frames[f], 0, 0, ccm, mode=MODE)
        want_total += r
        assert masks[f] == want_mask, f"frame {f}: mask {masks[f]:#x} vs {want_mask:#x}"
        assert (chunks[f] == want_chunks).all(), f"frame {f}: chunk bytes differ"
    assert total == want_total

    # every block's bytes where they fall (Decoder::decode into a plain stream): the corrected message, or zeros for a failed block
    dec.reset_ccm()
    r, data, ok = dec.decode_plain_batch(frames, color_correction=0)
    assert (ok == rs_ok).all()
    assert (data.reshape(nframes, B, k) == want_plain).all()


@functools.lru_cache(maxsize=None)
def one_bad_block_set(mode):
    """clean payload frames (valid fountain headers), frame i with exactly one block made uncorrectable (parity + 1 errors): the first and the
    last block of every chunk -- so in modes 68 / 67 / 66 every header-carrying block of the symbol stream -- and in mode 8 also block 64, the
    first one k_frame_end takes from its second ballot"""
    synth = framegen.FrameSynth("cpu", mode)
    geo = synth.geo
    n, p, B, C = geo.RS_BLOCK, geo.RS_PARITY, geo.BLOCKS, geo.CHUNKS_PER_FRAME
    BPC = B // C
    targets = sorted({c * BPC for c in range(C)} | {c * BPC + BPC - 1 for c in range(C)} | ({64} if mode == 8 else set()))
    nf = len(targets)
    payload = framegen.synth_payload(nf, seed=700 + mode, mode=mode)
    blocks = rs_cases.encode(payload.numpy().reshape(nf * B, geo.RS_DATA), p).reshape(nf, B, n)
    g = np.random.default_rng(800 + mode)
    for i, b in enumerate(targets):
        pos = g.choice(n, p + 1, replace=False)
        blocks[i, b, pos] ^= g.integers(1, 256, p + 1, dtype=np.uint8)
    frames = synth.render(rs_cases.blocks_to_tiles(synth, blocks)).numpy()
    return synth, targets, payload.numpy(), blocks, frames


def test_one_failed_block_per_frame_at_chunk_boundaries(dec, MODE):
    synth, targets, payload, blocks, frames = one_bad_block_set(MODE)
    geo = synth.geo
    n, p, k, B, C = geo.RS_BLOCK, geo.RS_PARITY, geo.RS_DATA, geo.BLOCKS, geo.CHUNKS_PER_FRAME
    BPC = B // C
    nf = len(targets)
    O = pyref.oracle_lib(MODE)
    for i, b in enumerate(targets):
        assert _rs(O, blocks[i, b], n, p)[0] <= 0, f"frame {i}: block {b} was meant to be uncorrectable"
        if pyref.ref_lib() is not None:
            assert _ref_rs(blocks[i, b], n, p)[0] <= 0, f"frame {i}: block {b} was meant to be uncorrectable"

    # taps, CCM (carried frame to frame), masks and chunks against the oracle
    chunks, masks, _ = check(dec, list(frames), cc=2)
    rs_ok = dec.tap(D.TAP_RS_OK, nf)
    for i, b in enumerate(targets):
        want_ok = np.ones(B, np.uint8)
        want_ok[b] = 0
        assert (rs_ok[i] == want_ok).all(), f"frame {i}: block flags {rs_ok[i]} (bad block {b})"
        # aligned_stream (aligned_stream.h:39-119): the chunk holding the bad block is lost; a bad LAST block of a chunk also leaves _badChunk
        # set for the next chunk, which is dropped too
        c = b // BPC
        lost = {c} | ({c + 1} if b % BPC == BPC - 1 and c + 1 < C else set())
        want_mask = geo.FULL_MASK & ~sum(1 << j for j in lost)
        assert masks[i] == want_mask, f"frame {i} (bad block {b}): mask {masks[i]:#x} vs {want_mask:#x}"
        for j in range(C):
            want = payload[i, j * geo.CHUNK:(j + 1) * geo.CHUNK] if j not in lost else np.zeros(geo.CHUNK, np.uint8)
            assert (chunks[i, j] == want).all(), f"frame {i} (bad block {b}): chunk {j}"

    # the plain stream: every block where it falls, the bad one as zero bytes
    dec.reset_ccm()
    r, data, ok = dec.decode_plain_batch(frames)
    ccm = pyref.CoCcm()
    want_r = 0
    for i, b in enumerate(targets):
        wr, wdata, wok, ccm = pyref.oracle_decode_plain(frames[i], 0, 2, ccm, mode=MODE)
        want_r += wr
        assert (ok[i] == wok).all() and (data[i] == wdata).all(), f"frame {i} (bad block {b})"
        want = payload[i].reshape(B, k).copy()
        want[b] = 0
        assert (data[i].reshape(B, k) == want).all(), f"frame {i} (bad block {b})"
    assert r == want_r


def test_pipelined_entry_on_fuzz_frames(dec, MODE):
    """the fuzz frames through decode_batch_pipelined (device buffers, two batches in flight) == decode_batch of the same frames"""
    synth, cases, blocks, frames = fuzz_set(MODE)
    geo = synth.geo
    nframes = frames.shape[0]
    dec.reset_ccm()
    _, want_chunks, want_masks = dec.decode_batch(frames, color_correction=0)
    dev = torch.device("cuda", 0)
    h = nframes // 2
    parts = [(0, h), (h, nframes)]
    d_in = [torch.from_numpy(np.ascontiguousarray(frames[a:b])).to(dev) for a, b in parts]
    d_ch = [torch.zeros((b - a, geo.FRAME_BYTES), dtype=torch.uint8, device=dev) for a, b in parts]
    d_mk = [torch.zeros(b - a, dtype=torch.int32, device=dev) for a, b in parts]
    st = torch.cuda.current_stream(dev).cuda_stream
    dec.reset_ccm()
    for (a, b), x, c, m in zip(parts, d_in, d_ch, d_mk):
        dec.decode_batch_pipelined(x.data_ptr(), b - a, c.data_ptr(), m.data_ptr(), False, 0, st)
    dec.pipeline_wait(st)
    torch.cuda.synchronize()
    got_chunks = torch.cat(d_ch).cpu().numpy()
    got_masks = torch.cat(d_mk).cpu().numpy().astype(np.uint32)
    assert (got_masks == want_masks).all(), f"masks {got_masks} vs {want_masks}"
    assert (got_chunks == want_chunks.reshape(nframes, -1)).all(), "chunk bytes differ"
