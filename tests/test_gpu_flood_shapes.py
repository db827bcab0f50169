"""GPU: the exact flood replay (k_flood3) in every launch shape the host picks from the number of frames -- three, four and eight frames
per CU, with and without the counter hand-out, on the two streams of a split batch, on four pipelined sets in flight at once, in every
mode's geometry. The other flood tests replay at most 160 frames per call, which is always the three-per-CU instance or a forced dense one.

A pool of six frames (five that leave the fast path in different ways, one clean) is decoded alone and held against the oracle frame by
frame: symbols, drifted positions, colours, masks, chunks. Large batches are that pool tiled on the device, and every frame of them must
come out as its pool frame did (colour correction off: no frame's result depends on its neighbours). Every call's launch records
(HipDecoder.tap_flood_launches) must be what tests/flood_launch_model.py predicts, and with the batch-parallel pass off every flagged frame
must report the exact replay -- so the instance the record names is the code that produced the compared cells."""
import contextlib
import os

import numpy as np
import pytest
import torch

from libcimbar_amd import decoder as D
from libcimbar_amd import framegen, geometry
from oracle import pyref
from tests import flood_launch_model as M
from tests import frames as F

pytestmark = pytest.mark.gpu

HEAP_LDS4, HEAP_LDS8 = 7080, 4095            # heap slots in LDS of the four-per-CU and the dense instance (k2b_flood.hip.inc)
DEPTH4 = {"CIMBAR_HIP_PIPE_DEPTH": "4", "CIMBAR_HIP_FLOOD_WAVE": "0"}     # A = 256, A3 = 192; every flagged frame takes the exact replay


@contextlib.contextmanager
def decoder(env, mode=68):
    """a context created under `env` (the library reads its switches at create)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dec = D.HipDecoder(0, mode)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield dec
    finally:
        torch.cuda.synchronize()
        dec.close()


def make_pool(mode):
    synth = framegen.FrameSynth("cpu", mode)
    h, w = synth.geo.IMG_H, synth.geo.IMG_W
    if mode != 68:
        payload, fr = F.clean_frames(synth, 3, seed=600 + mode)
        return [F.shift(fr[0], 2, 1), F.add_noise(F.shift(fr[1], -3, 2), 40, 7), fr[2]], ["shift", "shift+noise", "clean"]
    payload, fr = F.clean_frames(synth, 6, seed=291)
    rng = np.random.default_rng(13)
    return [
        F.shift(fr[0], 2, 1),                                             # clean rigid shift: the deepest heap
        F.add_noise(F.shift(fr[1], -3, 2), 40, 7),                        # mixed priorities, stale entries
        F.rescale(fr[2], 6),                                              # drift grows across the frame
        rng.integers(0, 256, (h, w, 3), dtype=np.uint8),                  # pure noise
        F.blank_region(F.shift(fr[4], 1, 1), 300, 420, 0, w),             # a shift with a wiped band
        fr[5],                                                            # untouched: flag 0, nothing to replay
    ], ["shift", "shift+noise", "rescale", "noise", "shift+band", "clean"]


_pools = {}


def pool(mode):
    """the mode's pool, what the oracle makes of every frame (colour correction off), and -- decoded alone with the batch-parallel pass off,
    held against the oracle -- what the library makes of it: computed once per mode and never changed"""
    if mode in _pools:
        return _pools[mode]
    frames, names = make_pool(mode)
    frames = np.ascontiguousarray(np.stack(frames))
    want, peaks = [], []
    for fr in frames:
        r, chunks, mask, _ = pyref.oracle_decode(fr, 0, 0, None, mode=mode)
        peaks.append(int(pyref.oracle_lib(mode).co_last_heap_peak()))             # (the oracle's symbol pass of this decode: tools/heap_peak.py)
        sym, col, pos = pyref.oracle_stage(mode=mode)
        want.append(dict(chunks=chunks.copy(), mask=mask, sym=sym, col=col, pos=pos))
    print(f"mode {mode} pool, oracle heap peaks:", dict(zip(names, peaks)))
    geo = geometry.for_mode(mode)
    if mode == 68:
        # conditions on the INPUT, checked before anything runs on the GPU: the four-per-CU and the dense instance really spill on this pool
        # (the clean frame is never replayed: its peak does not count)
        heap_cap = 12 * geo.NCELLS + 64
        replayed = [p for p, nm in zip(peaks, names) if nm != "clean"]
        assert sum(p > HEAP_LDS4 for p in replayed) >= 1 and sum(p > HEAP_LDS8 for p in replayed) >= 2 and max(peaks) < heap_cap, peaks
    n = len(frames)
    with decoder({"CIMBAR_HIP_FLOOD_WAVE": "0"}, mode) as dec:
        total, chunks, masks = dec.decode_batch(frames, color_correction=0)
        sym, col, drift, path = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_COLORS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_FLOOD_PATH, n)
        recs, reserved = dec.tap_flood_launches()
        assert (recs, reserved) == M.launches(n, "plain")
        xy = dec.geo.cell_positions()
    for k, w in enumerate(want):
        assert (sym[k] == w["sym"]).all(), f"{names[k]}: {(sym[k] != w['sym']).sum()} symbols differ"
        assert (xy + drift[k].astype(np.int32) == w["pos"]).all(), f"{names[k]}: drifted positions differ"
        assert (col[k] == w["col"]).all(), f"{names[k]}: colours differ"
        assert masks[k] == w["mask"] and (chunks[k] == w["chunks"]).all(), names[k]
    assert path.tolist() == [0 if nm == "clean" else 1 for nm in names], path
    dev = torch.device("cuda", 0)
    _pools[mode] = dict(frames=frames, names=names, peaks=peaks, sym=sym, drift=drift, path=path, masks=masks.astype(np.uint32),
                        chunks=chunks.reshape(n, -1), dev=torch.from_numpy(frames).to(dev), geo=geo)
    return _pools[mode]


class Batch:
    """n frames pool[(k + start) % len(pool)] on the device, with output buffers of their own"""

    def __init__(self, P, n, start=0):
        dev = P["dev"].device
        self.P, self.n = P, n
        self.idx = (np.arange(n) + start) % len(P["frames"])
        self.frames = P["dev"][torch.from_numpy(self.idx).to(dev)].contiguous()
        self.chunks = torch.zeros((n, P["geo"].FRAME_BYTES), dtype=torch.uint8, device=dev)
        self.masks = torch.zeros((n,), dtype=torch.int32, device=dev)

    def args(self):
        return self.frames.data_ptr(), self.n, self.chunks.data_ptr(), self.masks.data_ptr(), False, 0, torch.cuda.current_stream().cuda_stream

    def check_outputs(self, tag):
        """chunks and masks of every frame against its pool frame's"""
        P = self.P
        masks = self.masks.cpu().numpy().astype(np.uint32)
        bad = np.nonzero(masks != P["masks"][self.idx])[0]
        assert bad.size == 0, f"{tag}: masks differ in frames {bad[:8]} ({[P['names'][self.idx[k]] for k in bad[:8]]})"
        diff = (self.chunks.cpu().numpy() != P["chunks"][self.idx]).any(1)
        assert not diff.any(), f"{tag}: chunk bytes differ in frames {np.nonzero(diff)[0][:8]}"

    def check_taps(self, dec, tag, wave):
        """symbols, drift and path of every frame of the batch the context decoded last against its pool frame's"""
        P, n, idx = self.P, self.n, self.idx
        sym, drift, path = dec.tap(D.TAP_SYMBOLS, n), dec.tap(D.TAP_DRIFT, n), dec.tap(D.TAP_FLOOD_PATH, n)
        diff = (sym != P["sym"][idx]).any(1)
        assert not diff.any(), f"{tag}: symbols differ in frames {np.nonzero(diff)[0][:8]} of {int(diff.sum())}"
        # (the fast path decodes every cell at drift (0, 0) and never writes the drift buffer -- whoever reads it tests the flag first -- so a
        # clean frame's TAP_DRIFT is whatever the scratch set held before: there is nothing to compare)
        flagged = P["path"][idx] != 0
        diff = (drift != P["drift"][idx]).any((1, 2)) & flagged
        assert not diff.any(), f"{tag}: drift differs in frames {np.nonzero(diff)[0][:8]} of {int(diff.sum())}"
        if wave:
            # the batch-parallel pass may take what it can certify (2); it must not change which frames leave the fast path, nor any cell
            assert ((path != 0) == flagged).all() and (path <= 2).all(), f"{tag}: paths {np.bincount(path)}"
        else:
            assert (path == P["path"][idx]).all(), f"{tag}: paths differ in frames {np.nonzero(path != P['path'][idx])[0][:8]}"
            assert int((path == 1).sum()) == int(flagged.sum()) > 0
        return path


def areas_held(dec):
    """the spill areas the context holds now (the header record of TAP_FLOOD_LAUNCH)"""
    return int(dec.tap(D.TAP_FLOOD_LAUNCH, 0)[0, 1])


def pipelined(dec, batches, depth, first_call, tag, wave=False, held=None, **model):
    """issue every batch without waiting, reading the launch records after each call; then wait and compare every frame.
    first_call: how many pipelined calls the context has seen (call k runs on set (k + 1) % depth)."""
    st = torch.cuda.current_stream().cuda_stream
    for k, b in enumerate(batches):
        b.chunks.zero_(); b.masks.zero_()                                    # (what an earlier call left in them proves nothing)
        dec.decode_batch_pipelined(*b.args())
        got = dec.tap_flood_launches()                                       # (host bookkeeping: does not wait for the batches in flight)
        want = M.launches(b.n, "pipelined", pipe_depth=depth, pipe_set=(first_call + k + 1) % depth, **model)
        assert got == want, f"{tag} call {k}: launches {got}, the model says {want}"
        # held: the context must not have grown for this call -- growing waits for the whole device, and the batches would not be in flight together
        assert held is None or areas_held(dec) == held, f"{tag} call {k}: the context grew from {held} to {areas_held(dec)} areas"
        print(f"{tag} call {first_call + k}: {got}")
    dec.pipeline_wait(st)
    torch.cuda.synchronize()
    for k, b in enumerate(batches):
        b.check_outputs(f"{tag} batch {k}")
    return batches[-1].check_taps(dec, tag, wave)                            # (the taps describe the batch issued last: in_flight_every_way)


def in_flight_every_way(env, P, sizes, tag, **model):
    """one batch per pipelined set, all in flight at once -- as often as there are sets, on a fresh context each time, after depth, depth + 1, ...
    priming calls and with the issue order rotated as far: the taps read the set issued last, so every batch is once the one whose symbols, drift
    and paths are compared (every replayed frame on path 1) while the others run beside it, and every set is once the set it runs on.
    The priming calls decode the batch with the largest reservation, at least once on every set and waited for: a context that has to grow -- its
    spill areas (ensure_flood_areas waits for the device) or a set's scratch -- serialises the calls, so all growing is done before the group and
    the areas held are asserted not to change while it is issued."""
    depth = len(sizes)
    batches = [Batch(P, n, start=j) for j, n in enumerate(sizes)]
    largest = max(batches, key=lambda b: (M.launches(b.n, "pipelined", pipe_depth=depth, **model)[1], b.n))
    assert largest.n == max(sizes)                                             # (it also sizes every set's scratch for every batch of the group)
    tapped = set()
    for w in range(depth):
        with decoder(env) as dec:
            assert dec.pipeline_depth == depth
            for call in range(depth + w):
                pipelined(dec, [largest], depth, call, f"{tag}, priming", **model)
            held = areas_held(dec)
            assert held == max(M.launches(n, "pipelined", pipe_depth=depth, **model)[1] for n in sizes)
            order = [(w + i) % depth for i in range(depth)]
            pipelined(dec, [batches[j] for j in order], depth, depth + w, f"{tag}, order {order}", held=held, **model)
            tapped.add((order[-1], dec.tap_flood_launches()[0][0]["counter"]))
    # (batch, set) of the compared one: every batch once, every set once
    assert sorted(j for j, k in tapped) == sorted(k for j, k in tapped) == list(range(depth)), tapped


@pytest.mark.parametrize("n,instance,grid", [(192, 3, 192), (193, 4, 193), (256, 4, 256), (257, 8, 257)])
def test_pipelined_set_at_its_instance_boundaries(n, instance, grid):
    """A = 256: the last three-per-CU launch, the first and the last four-per-CU one with a workgroup per frame, the first dense one"""
    P = pool(68)
    with decoder(DEPTH4) as dec:
        assert dec.pipeline_depth == 4
        b = Batch(P, n)
        for call in range(2):                                                # twice on one context: sets 1 and 2
            pipelined(dec, [b], 4, call, f"{n} frames")
            rec = dec.tap_flood_launches()[0][0]
            assert (rec["instance"], rec["grid"], rec["frames"], rec["flags"]) == (instance, grid, n, 0)


def test_four_per_cu_with_frames_handed_out_by_the_counter():
    """300 frames on a set of 256 areas with the dense instance switched off: 256 workgroups, 44 frames through the counter pair -- five calls,
    so that the fifth finds the pair the first one used"""
    P = pool(68)
    with decoder({**DEPTH4, "CIMBAR_HIP_FLOOD_DENSE": "0"}) as dec:
        for call in range(5):
            pipelined(dec, [Batch(P, 300, start=call)], 4, call, "300 frames, no dense", dense=0)
            rec = dec.tap_flood_launches()[0][0]
            assert (rec["instance"], rec["grid"], rec["frames"], rec["counter"]) == (4, 256, 300, (call + 1) % 4)


def test_four_sets_in_flight_with_their_own_areas_and_counters():
    """4 x 300 frames, the dense instance off: 256 workgroups and a hand-out on every set at the same time"""
    P = pool(68)
    in_flight_every_way({**DEPTH4, "CIMBAR_HIP_FLOOD_DENSE": "0"}, P, [300] * 4, "4 x 300 frames", dense=0)
    seen = [M.launches(300, "pipelined", pipe_depth=4, pipe_set=k, dense=0)[0][0] for k in range(4)]
    assert [r["area0"] for r in seen] == [0, 256, 512, 768] and [r["counter"] for r in seen] == [0, 1, 2, 3]


def test_a_dense_set_in_flight_beside_an_ordinary_one():
    """default settings: 300 frames on one set take the dense instance (300 areas from the set's base), 200 frames on the next the four-per-CU
    one, both spilling -- their areas must not meet (they did while the ordinary instances counted their bases in single areas and the dense
    one in pairs: tests/test_flood_launch_model.py). Of the four rotations, the second issues the 300 frames last (set 1, the 200 on set 2
    issued three calls before) and compares their cells, the third the 200 (set 2, right behind the 300 on set 1): under the old bases both
    pairs shared areas [512, 712). The context is sized before each group (in_flight_every_way), so no call of it waits for the device."""
    P = pool(68)
    sizes = [300, 200, 257, 256]
    in_flight_every_way(DEPTH4, P, sizes, "300 dense | 200 | 257 dense | 256")
    for w in range(4):
        recs = [M.launches(sizes[(w + i) % 4], "pipelined", pipe_depth=4, pipe_set=(w + i + 1) % 4)[0][0] for i in range(4)]
        assert sorted(r["instance"] for r in recs) == [4, 4, 8, 8]
        spans = sorted((r["area0"], r["area0"] + r["grid"]) for r in recs)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans


def test_flags_of_every_kind_in_one_four_per_cu_launch():
    """the batch-parallel pass on (the default): certified frames (2), clean ones (0) and frames to replay (1) side by side in one launch"""
    P = pool(68)
    env = {"CIMBAR_HIP_PIPE_DEPTH": "4"}
    with decoder(env) as dec:
        path = pipelined(dec, [Batch(P, 193)], 4, 0, "193 frames, wave on", wave=True)
        assert dec.tap_flood_launches()[0][0]["instance"] == 4
        assert all(int((path == v).sum()) >= 1 for v in (0, 1, 2)), np.bincount(path)


@pytest.mark.parametrize("wave", [True, False])
def test_plain_batch_split_then_unsplit(wave):
    """770 frames through decode_batch_device on a fresh context: 385 + 385 on two streams, four per CU on both (384 < 385 <= 512), each in
    its own half of the areas; the same batch again runs as ONE chain (more than a quarter of the batch before took a flood kernel):
    768 < 770 <= 1024, four per CU"""
    P = pool(68)
    n = 770
    with decoder({} if wave else {"CIMBAR_HIP_FLOOD_WAVE": "0"}) as dec:
        b = Batch(P, n)
        mostly = False
        for call in range(2):
            b.chunks.zero_(); b.masks.zero_()
            dec.decode_batch_device(*b.args())
            got = dec.tap_flood_launches()
            torch.cuda.synchronize()
            want = M.launches(n, "plain", mostly_flood=mostly)
            print(f"plain 770, wave {wave}, call {call}: {got}")
            assert got == want, f"call {call}: launches {got}, the model says {want}"
            assert [(r["instance"], r["grid"], r["area0"], r["counter"]) for r in got[0]] == \
                ([(4, 385, 0, 0), (4, 385, 1024, 1)] if call == 0 else [(4, 770, 0, 0)])
            b.check_outputs(f"call {call}")
            path = b.check_taps(dec, f"call {call}", wave)
            mostly = 4 * int((path != 0).sum()) > n                            # what the next call reads of this one
        assert mostly


@pytest.mark.parametrize("mode", [67, 66])
def test_four_per_cu_in_the_other_geometries(mode):
    """the LDS budget of four workgroups per CU with each mode's own cell count: the mode's pool against its oracle, then 193 frames of it"""
    P = pool(mode)
    with decoder(DEPTH4, mode) as dec:
        pipelined(dec, [Batch(P, 193)], 4, 0, f"mode {mode}, 193 frames")
        rec = dec.tap_flood_launches()[0][0]
        assert (rec["instance"], rec["grid"]) == (4, 193)
