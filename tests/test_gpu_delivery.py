"""GPU: cimbar_hip_deliver_chunks / _delivery_reset / _delivery_stats against tests/delivery_model.py, byte for byte in packed[:count * cs],
src[:count] and count, through host memory and through device memory on a stream of its own, in all five modes. Inputs are synthetic slots and
masks (random bytes, crafted headers, fixed seeds); only the last test decodes anything. Every output buffer is filled with 0xA5 first and must
still hold it past what the call delivered."""
import ctypes

import numpy as np
import pytest
import torch

from libcimbar_amd import HipDecoder, decoder, geometry
from tests import delivery_model as dm

pytestmark = pytest.mark.gpu

MODES = (68, 67, 66, 4, 8)
GUARD_WORD = np.frombuffer(b"\xA5" * 4, np.int32)[0]
ALL = dm.DEDUP | dm.DROP_EMPTY

_decoders = {}


def dec_for(mode):
    if mode not in _decoders:
        _decoders[mode] = HipDecoder(0, mode)
    return _decoders[mode]


def shape_of(mode):
    g = geometry.for_mode(mode)
    return g.CHUNKS_PER_FRAME, g.CHUNK


def random_slots(mode, n, seed):
    """random bytes whose headers are all distinct and none empty: b0 has the size bit, b2..b5 count up"""
    per, cs = shape_of(mode)
    rng = np.random.default_rng(seed)
    chunks = rng.integers(0, 256, (n, per, cs), dtype=np.uint8)
    ids = np.arange(n * per, dtype=np.uint32).reshape(n, per) + np.uint32(seed << 20)
    chunks[:, :, 0] = 0x89
    chunks[:, :, 1] = 0x01
    for b in range(4):
        chunks[:, :, 2 + b] = (ids >> (8 * (3 - b))) & 0xFF
    return chunks


def run_host(dec, chunks, masks, flags, want_src=True):
    n, per, cs = chunks.shape
    packed = np.full(n * per * cs, 0xA5, np.uint8)
    src = np.full(n * per, GUARD_WORD, np.int32)
    count = ctypes.c_int32(-1)
    rc = dec._lib.cimbar_hip_deliver_chunks(dec._ctx, chunks.ctypes.data, masks.ctypes.data, n, decoder.MEM_HOST, flags, packed.ctypes.data,
                                            src.ctypes.data if want_src else None, ctypes.addressof(count), decoder.MEM_HOST, None)
    dec._check(rc, "cimbar_hip_deliver_chunks")
    assert rc == count.value
    return packed, src, int(rc)


def run_device(dec, chunks, masks, flags, want_src=True):
    n, per, cs = chunks.shape
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_c = torch.from_numpy(chunks).to(dev)
        d_m = torch.from_numpy(masks.view(np.int32)).to(dev)
        d_p = torch.full((n * per * cs,), 0xA5, dtype=torch.uint8, device=dev)
        d_s = torch.full((n * per,), int(GUARD_WORD), dtype=torch.int32, device=dev)
        d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
        dec.deliver_chunks_device(d_c.data_ptr(), d_m.data_ptr(), n, d_p.data_ptr(), d_s.data_ptr() if want_src else None, d_n.data_ptr(),
                                  stream=st.cuda_stream, flags=flags)
    st.synchronize()
    return d_p.cpu().numpy(), d_s.cpu().numpy(), int(d_n.cpu()[0])


def check(got, want, cs, want_src=True):
    packed, src, count = got
    wp, ws = want
    assert count == len(ws)
    assert (packed[:count * cs].reshape(count, cs) == wp).all()
    assert (packed[count * cs:] == 0xA5).all()                       # nothing written past what was delivered
    if want_src:
        assert (src[:count] == ws).all() and (src[count:] == GUARD_WORD).all()
    else:
        assert (src == GUARD_WORD).all()


def both_paths(dec, model_factory, chunks, masks, flags):
    """one model per path: each path runs on its own remembered state only where the caller resets in between (REMEMBER tests do it by hand)"""
    cs = chunks.shape[2]
    want = model_factory().deliver(chunks, masks, flags)
    check(run_host(dec, chunks, masks, flags), want, cs)
    check(run_device(dec, chunks, masks, flags), want, cs)
    return want


@pytest.mark.parametrize("mode", MODES)
def test_boundary_sizes(mode):
    dec = dec_for(mode)
    per, cs = shape_of(mode)
    full = np.uint32((1 << per) - 1)
    for flags in (0, ALL):
        one = random_slots(mode, 1, 1)
        p, s = both_paths(dec, dm.DeliveryModel, one, np.zeros(1, np.uint32), flags)                    # nothing delivered, nothing written
        assert len(s) == 0
        for slot in (0, per - 1):
            p, s = both_paths(dec, dm.DeliveryModel, one, np.array([1 << slot], np.uint32), flags)
            assert s.tolist() == [slot]
        for n in (2, 3):          # every output index, so every alignment of the chunk size modulo 4, source and destination
            p, s = both_paths(dec, dm.DeliveryModel, random_slots(mode, n, 2), np.full(n, full, np.uint32), flags)
            assert len(s) == n * per
    rng = np.random.default_rng(3)
    for n in (65, 257):           # across a wavefront and across four of the scan's sixteen (its rounds of 1024 frames: test_scan_rounds)
        masks = rng.integers(0, 1 << per, n, dtype=np.uint32)
        masks[rng.integers(0, n, n // 8)] = 0
        both_paths(dec, dm.DeliveryModel, random_slots(mode, n, 4), masks, ALL)
    # src may be NULL
    chunks, masks = random_slots(mode, 3, 5), np.array([5, 0, full], np.uint32)
    want = dm.DeliveryModel().deliver(chunks, masks, ALL)
    check(run_host(dec, chunks, masks, ALL, want_src=False), want, cs, want_src=False)
    check(run_device(dec, chunks, masks, ALL, want_src=False), want, cs, want_src=False)


@pytest.mark.parametrize("mode", MODES)
def test_duplicates(mode):
    dec = dec_for(mode)
    per, cs = shape_of(mode)
    full = np.uint32((1 << per) - 1)
    # within one frame
    c = random_slots(mode, 1, 6)
    c[0, per - 1, :6] = c[0, 1, :6]
    c[0, 2, :6] = c[0, 1, :6]
    _, s = both_paths(dec, dm.DeliveryModel, c, np.array([full], np.uint32), ALL)
    assert s.tolist() == [j for j in range(per) if j not in (2, per - 1)]
    # in the first and the last frame of 257
    c = random_slots(mode, 257, 7)
    c[256, per - 1, :6] = c[0, 0, :6]
    c[256, 0, :6] = c[0, per - 1, :6]
    c[0, 1, :6] = c[0, 0, :6]
    _, s = both_paths(dec, dm.DeliveryModel, c, np.full(257, full, np.uint32), ALL)
    assert len(s) == 257 * per - 3 and s[0] == 0 and s[1] == 2
    # every candidate the same header: the lowest candidate alone
    c = random_slots(mode, 65, 8)
    c[:, :, :6] = c[3, 1, :6]
    masks = np.full(65, full, np.uint32)
    masks[:3] = 0
    masks[3] = full & ~np.uint32(3)
    p, s = both_paths(dec, dm.DeliveryModel, c, masks, ALL)
    assert s.tolist() == [3 * per + 2] and (p[0] == c[3, 2]).all()


def test_many_headers_each_twice_exercise_probing():
    """513 frames of mode 68: 3078 headers that count up the way block ids do, every one of them on two slots a random distance apart"""
    dec = dec_for(68)
    per, cs = shape_of(68)
    n = 513
    c = random_slots(68, n, 9)
    flat = c.reshape(n * per, cs)
    perm = np.random.default_rng(10).permutation(n * per)
    flat[perm[n * per // 2:], :6] = flat[perm[:n * per // 2], :6]
    p, s = both_paths(dec, dm.DeliveryModel, c, np.full(n, 0xFFF, np.uint32), ALL)
    assert len(s) == n * per // 2


@pytest.mark.parametrize("mode", (68, 66))
def test_headers_one_byte_apart(mode):
    dec = dec_for(mode)
    per, cs = shape_of(mode)
    base = [0x91, 0x22, 0x33, 0x44, 0x55, 0x66]
    c = random_slots(mode, 3, 11)
    for byte in range(6):                 # base, then its six neighbours, then all seven again
        other = list(base)
        other[byte] ^= 0x01
        c.reshape(-1, cs)[1 + byte, :6] = other
        c.reshape(-1, cs)[8 + byte, :6] = other
    c.reshape(-1, cs)[0, :6] = base
    c.reshape(-1, cs)[7, :6] = base
    masks = np.zeros(3, np.uint32)
    for i in range(14):
        masks[i // per] |= np.uint32(1 << (i % per))
    _, s = both_paths(dec, dm.DeliveryModel, c, masks, ALL)
    assert s.tolist() == list(range(7))


@pytest.mark.parametrize("mode", MODES)
def test_drop_empty(mode):
    dec = dec_for(mode)
    per, cs = shape_of(mode)
    c = random_slots(mode, 4, 12)
    c[1] = 0                                              # a too-small frame: all-zero chunks, every bit set
    c[2, 0, :6] = [0x80, 0, 0, 0, 0, 0]                   # the size's top bit alone: not empty
    c[2, 1, :6] = [0x80, 0, 0, 0, 0, 0]
    c[2, 2, :6] = [0x7F, 0, 0, 0, 3, 4]                   # an encode id and a block id, size 0: empty
    c[3, per - 1] = 0
    masks = np.full(4, (1 << per) - 1, np.uint32)
    _, s = both_paths(dec, dm.DeliveryModel, c, masks, ALL)
    assert len(s) == 4 * per - per - 1 - 1 - 1
    _, s = both_paths(dec, dm.DeliveryModel, c, masks, dm.DROP_EMPTY)
    assert len(s) == 4 * per - per - 1 - 1
    _, s = both_paths(dec, dm.DeliveryModel, c, masks, dm.DEDUP)          # the empty header is then a header like any other
    assert len(s) == 4 * per - (per - 1) - 1 - 1
    _, s = both_paths(dec, dm.DeliveryModel, c, masks, 0)
    assert len(s) == 4 * per


def remember_sequence(dec, run, mode=68):
    """the calls of the REMEMBER test on one context through one path; returns everything it produced"""
    per, cs = shape_of(mode)
    full = np.uint32((1 << per) - 1)
    R = dm.REMEMBER | dm.DROP_EMPTY
    m = dm.DeliveryModel()
    out = []

    def step(chunks, masks, flags):
        want = m.deliver(chunks, masks, flags)
        got = run(dec, chunks, masks, flags)
        check(got, want, cs)
        assert dec.delivery_stats() == m.stats()
        out.append((got[0][:got[2] * cs].copy(), got[1][:got[2]].copy(), got[2], dec.delivery_stats()))
        return want

    dec.delivery_reset()
    m.reset()
    a = random_slots(mode, 5, 13)
    b = random_slots(mode, 5, 14)
    b[0, 1, :6] = a[4, per - 1, :6]
    b[2, :, :6] = a[1, :, :6]
    b[4, 0, :6] = b[3, 0, :6]                 # a duplicate inside the second call as well
    b[4, 2] = 0
    fullm = np.full(5, full, np.uint32)
    step(a, fullm, R)
    _, s = step(b, fullm, R)                  # seen and new headers mixed
    assert len(s) == 5 * per - 1 - per - 1 - 1
    _, s = step(b, fullm, ALL)                # a call without REMEMBER neither asks nor tells
    assert len(s) == 5 * per - 1 - 1
    dec.delivery_reset()
    m.reset()
    assert dec.delivery_stats() == (0, 1 << 20, False)
    _, s = step(b, fullm, R)                  # after the reset the second call keeps everything it can
    assert len(s) == 5 * per - 1 - 1

    # a table of 16 entries takes 8 headers
    dec.delivery_reset(4)
    m.reset(4)
    step(a[:1], np.array([0x1F], np.uint32), dm.REMEMBER)
    _, s = step(a[:1], np.array([0x3F], np.uint32) if per == 6 else np.array([0x1FF], np.uint32), dm.REMEMBER)
    if per > 6:
        assert s.tolist() == [5, 6, 7, 8] and m.stats() == (5, 16, True)       # 9 > 8: none remembered, none lost, the known ones still dropped
        _, s = step(a[:1], np.array([0x0E0], np.uint32), dm.REMEMBER)
        assert s.tolist() == [5, 6, 7] and m.stats() == (8, 16, True)          # sticky
    _, s = step(b[:2], np.array([full, full], np.uint32), dm.REMEMBER)         # more than 8 new headers in one call
    assert m.stats()[2] is True and len(s) >= 2 * per - 1 - per
    want_all = {dm.header_key(x) for x in b[:2].reshape(-1, cs)}
    assert want_all - m.seen <= {dm.header_key(x) for x in b[:2].reshape(-1, cs)[s]}   # no header that is not a duplicate is missing
    dec.delivery_reset(4)
    m.reset(4)
    assert dec.delivery_stats() == (0, 16, False)
    step(a[:1], np.array([0x7], np.uint32), dm.REMEMBER)
    dec.delivery_reset()
    return out


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("mode", (68, 66))
def test_remember(mode, path):
    remember_sequence(dec_for(mode), run_host if path == "host" else run_device, mode)



# ---- k_deliver_scan past its first round: one workgroup of 16 wavefronts scans 1024 frames a round and hands `carry` to the next
ROUND = 1024
SCAN_SIZES = (1023, 1024, 1025, 2047, 2049, 3000)


def scan_masks(mode, n, seed):
    """test_boundary_sizes' random masks, no chunk on frames 1020 .. 1030 except every chunk of 1023 and 1024 (the last lane of a round, the
    first of the next). Every wavefront 9 .. 15 of the first round keeps a chunk -- the slots of wsum[] nothing smaller reaches -- and every
    later round starts with a carry."""
    per, _ = shape_of(mode)
    rng = np.random.default_rng(seed)
    masks = rng.integers(0, 1 << per, n, dtype=np.uint32)
    masks[rng.integers(0, n, n // 8)] = 0
    masks[1020:1031] = 0
    masks[1023:1025] = (1 << per) - 1
    assert n >= ROUND - 1 and all(masks[64 * w:64 * w + 64].any() for w in range(9, 16))
    assert masks[:ROUND].any()                       # what the second round is handed is not zero
    return masks


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("mode", (66, 68))
def test_scan_rounds(mode, n):
    dec = dec_for(mode)
    per, cs = shape_of(mode)
    chunks, masks = random_slots(mode, n, 20), scan_masks(mode, n, 21 + n)
    for flags in (0, ALL):
        _, s = both_paths(dec, dm.DeliveryModel, chunks, masks, flags)
        assert len(s) == sum(bin(int(m)).count("1") for m in masks)           # (distinct headers, none empty: the masks alone decide)


def test_scan_rounds_benchmark_batch():
    """8192 frames of mode 68, 61 MB of slots: the batch benchmark config 4 delivers, eight rounds of the scan"""
    dec = dec_for(68)
    chunks, masks = random_slots(68, 8192, 22), scan_masks(68, 8192, 23)
    for flags in (0, ALL):
        both_paths(dec, dm.DeliveryModel, chunks, masks, flags)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("mode", (66, 68))
def test_remember_across_scan_rounds(mode, path):
    """two consecutive REMEMBER calls of 2049 and 3000 frames; a third of the second call's headers are the first call's"""
    dec, run = dec_for(mode), run_host if path == "host" else run_device
    per, cs = shape_of(mode)
    R = dm.REMEMBER | dm.DROP_EMPTY
    a, ma = random_slots(mode, 2049, 24), scan_masks(mode, 2049, 25)
    b, mb = random_slots(mode, 3000, 26), scan_masks(mode, 3000, 27)
    rng = np.random.default_rng(28)
    fa, fb = a.reshape(-1, cs), b.reshape(-1, cs)
    pick = rng.permutation(len(fb))[:len(fb) // 3]
    fb[pick, :6] = fa[rng.integers(0, len(fa), len(pick)), :6]
    m = dm.DeliveryModel()
    dec.delivery_reset()
    m.reset()
    try:
        counts = []
        for chunks, masks in ((a, ma), (b, mb)):
            want = m.deliver(chunks, masks, R)
            check(run(dec, chunks, masks, R), want, cs)
            assert dec.delivery_stats() == m.stats()
            counts.append(len(want[1]))
        assert counts[0] == sum(bin(int(x)).count("1") for x in ma) and 0 < counts[1] < sum(bin(int(x)).count("1") for x in mb)
        assert m.stats() == (counts[0] + counts[1], 1 << 20, False)
    finally:
        dec.delivery_reset()


def test_reset_refuses_a_capacity_out_of_range_and_unknown_flags():
    dec = dec_for(68)
    for bad in (1, 3, 25, -1):
        assert dec._lib.cimbar_hip_delivery_reset(dec._ctx, bad) == -1
    c, m = random_slots(68, 1, 15), np.array([1], np.uint32)
    packed, src, count = np.zeros(7500, np.uint8), np.zeros(12, np.int32), ctypes.c_int32(-7)

    def call(chunks=c.ctypes.data, masks=m.ctypes.data, n=1, in_mem=0, flags=0, p=packed.ctypes.data, cnt=ctypes.addressof(count), out_mem=0):
        return dec._lib.cimbar_hip_deliver_chunks(dec._ctx, chunks, masks, n, in_mem, flags, p, src.ctypes.data, cnt, out_mem, None)
    assert call() == 1
    for kw in (dict(chunks=None), dict(masks=None), dict(p=None), dict(cnt=None), dict(n=0), dict(n=-3), dict(flags=8), dict(flags=0x80000001),
               dict(in_mem=2), dict(out_mem=7), dict(n=(1 << 24) // 12 + 1)):
        count.value = -7
        assert call(**kw) == -1 and count.value == -7, kw


def test_determinism_on_fresh_contexts():
    """the n = 257 duplicate case and the REMEMBER sequence, twice, each time on a context of its own: identical outputs"""
    per, cs = shape_of(68)
    c = random_slots(68, 257, 16)
    flat = c.reshape(-1, cs)
    perm = np.random.default_rng(17).permutation(257 * per)
    flat[perm[1000:2000], :6] = flat[perm[:1000], :6]
    flat[perm[2000:3000], :6] = flat[perm[:1000], :6]
    masks = np.random.default_rng(18).integers(0, 1 << per, 257, dtype=np.uint32)
    runs = []
    for _ in range(2):
        dec = HipDecoder(0, 68)
        got = run_device(dec, c, masks, ALL)
        seq = remember_sequence(dec, run_device)
        runs.append((got, seq))
        dec.close()
    (g0, s0), (g1, s1) = runs
    assert g0[2] == g1[2] and (g0[0] == g1[0]).all() and (g0[1] == g1[1]).all()
    assert len(s0) == len(s1)
    for x, y in zip(s0, s1):
        assert x[2] == y[2] and x[3] == y[3] and (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_end_to_end_decode_then_deliver(ref):
    """8 encoded frames of a real fountain stream, 3 of them present twice, through decode_batch with device outputs and deliver_chunks_device on
    the same stream: one chunk per distinct header, equal to the model on the decode's own outputs, and food for the reference's sink"""
    from oracle.pyref import P
    dec = dec_for(68)
    per, cs = shape_of(68)
    dev = torch.device("cuda", 0)
    data = np.random.default_rng(19).integers(0, 256, 20000, dtype=np.uint8)
    stream = np.zeros((5 * per, cs), np.uint8)
    assert ref.ref_fountain_chunks(P(data), data.size, 9, 5 * per, P(stream)) == 5 * per
    order = [0, 1, 0, 2, 3, 1, 4, 3]
    payload = np.ascontiguousarray(stream.reshape(5, per * cs)[order])
    frames = dec.encode_batch(payload)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_f = torch.from_numpy(frames).to(dev)
        d_c = torch.zeros((8, per * cs), dtype=torch.uint8, device=dev)
        d_m = torch.zeros((8,), dtype=torch.int32, device=dev)
        d_p = torch.full((8 * per * cs,), 0xA5, dtype=torch.uint8, device=dev)
        d_s = torch.full((8 * per,), int(GUARD_WORD), dtype=torch.int32, device=dev)
        d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
        dec.reset_ccm()
        dec.decode_batch_device(d_f.data_ptr(), 8, d_c.data_ptr(), d_m.data_ptr(), False, 2, st.cuda_stream)
        dec.deliver_chunks_device(d_c.data_ptr(), d_m.data_ptr(), 8, d_p.data_ptr(), d_s.data_ptr(), d_n.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    chunks = d_c.cpu().numpy().reshape(8, per, cs)
    masks = d_m.cpu().numpy().view(np.uint32)
    assert (masks == 0xFFF).all() and (chunks.reshape(8, -1) == payload).all()
    count = int(d_n.cpu()[0])
    want = dm.DeliveryModel().deliver(chunks, masks, ALL)
    check((d_p.cpu().numpy(), d_s.cpu().numpy(), count), want, cs)
    assert count == len({dm.header_key(x) for x in stream}) == 5 * per
    packed = d_p.cpu().numpy()[:count * cs].reshape(count, cs)
    ref.ref_sink_reset(cs)
    results, out = [], np.zeros(data.size, np.uint8)
    for x in packed:
        r = int(ref.ref_sink_decode_frame(P(np.ascontiguousarray(x)), cs))
        results.append(r)
        if r > 0:                 # complete: the file is taken at once, as every caller of the sink does
            assert ref.ref_sink_recover(ctypes.c_uint32(r), P(out), out.size) == 1 and (out == data).all()
    assert -11 not in results and min(results) >= -1 and sum(1 for r in results if r > 0) == 1     # accepted piece by piece; the file completes
