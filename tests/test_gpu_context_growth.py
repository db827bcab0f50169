"""GPU: one context's buffers growing at different times. Every buffer of a context is grown on demand by whichever call needs it first, and the
pipelined entry point keeps one set of batch intermediates per batch in flight; whatever order the calls come in, a call returns what a FRESH
context returns for the plain, non-pipelined entry point on the same inputs with the same settings -- masks and chunk bytes exactly."""
import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen
from tests import frames as F

pytestmark = pytest.mark.gpu

# 1080p captures of a frame of the mode (tests/test_gpu_modes.py, tests/test_gpu_extract.py)
QUADS = {68: [((500, 40), (1480, 70), (470, 1030), (1500, 1000)), ((448, 28), (1472, 28), (448, 1052), (1472, 1052))],
         66: [((400, 60), (1500, 75), (395, 1010), (1510, 1000)), ((380, 40), (1540, 40), (380, 1044), (1540, 1044))]}


@pytest.fixture(scope="module", params=[68, 66])
def MODE(request):
    return request.param


@pytest.fixture(scope="module")
def pool(MODE):
    """(payload, clean frames, the frames the batches are made of): clean ones, ones that take the flood (rigid shifts, noise) and a blank one,
    which has no colour matrix of its own"""
    synth = framegen.FrameSynth("cpu", MODE)
    payload, clean = F.clean_frames(synth, 6, seed=314)
    mixed = [clean[0], F.shift(clean[1], 2, 1), F.add_noise(clean[2], 40, 1), clean[3], F.shift(clean[4], -1, 2), F.add_noise(clean[5], 60, 2),
             F.shift(clean[0], 1, 0)]
    return payload, clean, mixed, np.zeros_like(clean[0])


def same(got, want, tag):
    """tuples of arrays and numbers, exactly"""
    assert len(got) == len(want), tag
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{tag}: result {k} differs"
        else:
            assert g == w, f"{tag}: result {k}: {g} vs {w}"


def test_sets_that_grow_at_different_times(MODE, pool):
    """pipelined batches of unequal sizes: with three sets in rotation each set is regrown on a different call and small batches land on large
    sets; the colour-correction carry crosses from set to set, and the colour retry's margin buffer joins sets that already have their capacity"""
    _, _, mixed, blank = pool
    sizes = [1, 3, 2, 5, 1, 4, 6, 2]
    dev = torch.device("cuda", 0)
    batches = []
    for k, s in enumerate(sizes):
        fr = [mixed[(2 * k + j) % len(mixed)] for j in range(s)]
        if k in (2, 3, 5, 7):
            fr[0] = blank                      # no matrix of its own at the start of a batch: it takes the one the batch before left
        batches.append(torch.from_numpy(np.ascontiguousarray(np.stack(fr))).to(dev))
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(pipelined):
        dec = D.HipDecoder(0, MODE)
        if pipelined:
            assert dec.pipeline_depth == 3
        outs = [(torch.zeros((s, dec.geo.FRAME_BYTES), dtype=torch.uint8, device=dev), torch.zeros((s,), dtype=torch.int32, device=dev)) for s in sizes]
        flood = []
        for k, (t, (c, m)) in enumerate(zip(batches, outs)):
            if k == 4:
                dec.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)
            if pipelined:
                dec.decode_batch_pipelined(t.data_ptr(), sizes[k], c.data_ptr(), m.data_ptr(), False, 2, st)
            else:
                dec.decode_batch_device(t.data_ptr(), sizes[k], c.data_ptr(), m.data_ptr(), False, 2, st)
                torch.cuda.synchronize()
                flood.append(dec.tap(D.TAP_FLOOD, sizes[k]).copy())
        if pipelined:
            dec.pipeline_wait(st)
        torch.cuda.synchronize()
        res = [(c.cpu().numpy(), m.cpu().numpy()) for c, m in outs]
        ccm = dec.get_ccm()
        dec.close()
        return res, ccm, flood

    want, wccm, flood = run(False)
    assert sum(int(f.any()) for f in flood) >= 4, "the batches must hold frames that take the flood"
    got, gccm, _ = run(True)
    for k, ((wc, wm), (gc, gm)) in enumerate(zip(want, got)):
        assert (wm == gm).all(), f"batch {k}: masks {wm} vs {gm}"
        assert (wc == gc).all(), f"batch {k}: chunk bytes differ"
    assert wccm[0] == gccm[0] and wccm[1].tobytes() == gccm[1].tobytes()
    assert wccm[0], "the sequence must carry a matrix"


def test_one_context_through_every_buffer_family(MODE, pool):
    """every family of buffers grown once by a small call and again by a larger one, on ONE context; each result is what a fresh context gives for
    that call alone (the carried matrix reset on the old one first)"""
    payload, clean, mixed, blank = pool
    dec = D.HipDecoder(0, MODE)
    geo = dec.geo

    def both(tag, call):
        fresh = D.HipDecoder(0, MODE)
        want = call(fresh)
        fresh.close()
        dec.reset_ccm()
        got = call(dec)
        same(got, want, tag)
        return got

    frames = np.ascontiguousarray(np.stack([mixed[1], blank, clean[0], mixed[2], mixed[4]]))
    both("decode_batch n=1", lambda d: d.decode_batch(frames[:1]))
    first = both("decode_batch n=5", lambda d: d.decode_batch(frames))
    assert first[2][2] == geo.FULL_MASK and (first[1][2].reshape(-1) == payload[0]).all()

    # three captures of two frames, then six of three: the combined batch
    six = np.ascontiguousarray(np.stack([clean[0], F.add_noise(clean[0], 30, 7), clean[1], F.add_noise(clean[1], 30, 8), clean[2], F.add_noise(clean[2], 30, 9)]))
    both("decode_batch_combined n=3", lambda d: d.decode_batch_combined(six[:3]))
    both("decode_batch_combined n=6", lambda d: d.decode_batch_combined(six))

    cams = np.ascontiguousarray(np.stack([F.camera_frame(clean[k], quad=QUADS[MODE][k % 2], background=30 + 40 * k) for k in range(4)]))
    both("scan_extract_decode_batch n=2", lambda d: d.scan_extract_decode_batch(cams[:2]))
    caps = both("scan_extract_decode_batch n=4", lambda d: d.scan_extract_decode_batch(cams))
    assert (caps[2] == geo.FULL_MASK).sum() >= 2          # the captures do decode

    def in_flight(d):
        # more frames than the pipeline is deep: every slot is used, and used again; two in flight at a time
        out, tickets = [], []
        for k in range(d.pipeline_depth + 2):
            tickets.append(d.decode_frame_async(frames[k % len(frames)]))
            if len(tickets) > 1:
                out.extend(d.decode_frame_wait(tickets.pop(0)))
        out.extend(d.decode_frame_wait(tickets.pop(0)))
        return tuple(out)
    both("decode_frame_async / _wait", in_flight)

    # an image larger than the frame: the grid sits in its middle (the one-at-a-time path behind decode_frame)
    padded = np.zeros((geo.IMG_H + 16, geo.IMG_W + 36, 3), np.uint8)
    padded[8:8 + geo.IMG_H, 8:8 + geo.IMG_W] = clean[3]
    both("decode_frame, padded image", lambda d: d.decode_frame(padded))

    both("deliver_chunks", lambda d: d.deliver_chunks(first[1], first[2]))
    last = both("decode_batch n=2 again", lambda d: d.decode_batch(frames[2:4]))
    assert last[2][0] == geo.FULL_MASK and (last[1][0].reshape(-1) == payload[0]).all()
    dec.close()


def test_create_use_destroy(MODE, pool):
    """ten contexts one after the other, each closed with a pipelined batch still in flight: closing waits for it, and nothing of one context
    is in the way of the next"""
    payload, clean, _, _ = pool
    dev = torch.device("cuda", 0)
    two = np.ascontiguousarray(clean[:2])
    t = torch.from_numpy(np.ascontiguousarray(clean[2:5])).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for cycle in range(10):
        dec = D.HipDecoder(0, MODE)
        geo = dec.geo
        total, chunks, masks = dec.decode_batch(two)
        assert total == 2 * geo.FRAME_BYTES and (masks == geo.FULL_MASK).all() and (chunks.reshape(2, -1) == payload[:2]).all(), cycle
        c = torch.zeros((3, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
        m = torch.zeros((3,), dtype=torch.int32, device=dev)
        dec.decode_batch_pipelined(t.data_ptr(), 3, c.data_ptr(), m.data_ptr(), False, 2, st)
        dec.close()                                            # (no pipeline_wait)
        assert (m.cpu().numpy() == geo.FULL_MASK).all() and (c.cpu().numpy() == payload[2:5]).all(), cycle
