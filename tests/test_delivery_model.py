"""Chunk delivery, the rules (tests/delivery_model.py) without a GPU: against the reference's fountain_decoder_sink, case by case, and the argument
checks of the C call that run before any device work."""
import ctypes

import numpy as np
import pytest

from oracle.pyref import P
from tests import delivery_model as dm

PER, CS = 12, 625


def crafted(n, headers, seed=0, per=PER, cs=CS):
    """n frames of random bytes; headers: {(frame, slot): six bytes}"""
    rng = np.random.default_rng(seed)
    chunks = rng.integers(0, 256, (n, per, cs), dtype=np.uint8)
    chunks[:, :, 0] |= 0x80          # never empty by accident
    for (f, j), h in headers.items():
        chunks[f, j, :6] = h
    return chunks


def test_model_against_the_reference_sink(ref):
    """a fountain stream whose frames each arrive two or three times, with chunks missing here and there and all-zero chunks among them: the sink
    fed the model's packed output completes on the same chunk as the sink fed every masked slot, and recovers the same file"""
    rng = np.random.default_rng(77)
    size = 24000                                          # 39 wirehair blocks of 619 bytes: complete after ~4 of the 6 distinct frames
    data = rng.integers(0, 256, size, dtype=np.uint8)
    stream = np.zeros((6 * PER, CS), np.uint8)
    assert ref.ref_fountain_chunks(P(data), size, 9, 6 * PER, P(stream)) == 6 * PER
    stream = stream.reshape(6, PER, CS)
    order = [0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 5]   # every frame present two or three times
    chunks = np.ascontiguousarray(stream[order])
    masks = np.full(len(order), 0xFFF, np.uint32)
    for f in range(len(order)):                           # a different chunk or two missing from every capture
        for j in rng.choice(PER, 2, replace=False):
            masks[f] &= ~np.uint32(1 << int(j))
    for f, j in [(0, 3), (2, 0), (7, 11), (8, 11)]:       # the all-zero chunks of a too-small frame, delivered with their bit set
        chunks[f, j] = 0
        masks[f] |= np.uint32(1 << j)

    def feed(pieces):
        ref.ref_sink_reset(CS)
        results, done_on, out = [], None, np.zeros(size, np.uint8)
        for c in pieces:
            r = int(ref.ref_sink_decode_frame(P(np.ascontiguousarray(c)), CS))
            results.append(r)
            if r > 0:            # complete: take the file at once, as every caller of the sink does (the stream is then marked done)
                assert done_on is None
                done_on = (r, bytes(c[:6]))
                assert ref.ref_sink_recover(ctypes.c_uint32(r), P(out), size) == 1
                assert ref.ref_sink_is_done(ctypes.c_uint32(r)) == 1
        assert done_on is not None, results
        return results, done_on, out

    walk = dm.slot_walk(chunks, masks)
    res_all, done_all, out_all = feed(walk)
    packed, src = dm.DeliveryModel().deliver(chunks, masks, dm.DEDUP | dm.DROP_EMPTY)
    res_packed, done_packed, out_packed = feed(packed)
    assert done_packed == done_all and (out_packed == out_all).all() and (out_all == data).all()
    assert -11 not in res_packed and res_all.count(-11) == 4
    keys = [dm.header_key(c) for c in packed]
    assert len(set(keys)) == len(keys)                    # no header twice
    # every masked slot the model left out is one the first sink made no use of: refused as empty (-11), or a header it had been given before
    # (FountainDecoder::decode's set of seen block ids)
    linear = [f * PER + j for f in range(len(order)) for j in range(PER) if (int(masks[f]) >> j) & 1]
    kept, seen = set(src.tolist()), set()
    assert len(linear) == len(res_all) and kept <= set(linear)
    for i, r in zip(linear, res_all):
        k = dm.header_key(chunks.reshape(-1, CS)[i])
        if i not in kept:
            assert r == -11 or k in seen, (i, r)
        else:
            assert r != -11 and k not in seen, (i, r)
        if r != -11:
            seen.add(k)
    assert 0 < len(kept) < len(linear)


def test_flags_zero_is_the_receive_shims_loop():
    chunks = crafted(5, {(1, 2): [0] * 6, (3, 0): [1, 2, 3, 4, 5, 6], (4, 11): [1, 2, 3, 4, 5, 6]}, seed=1)
    masks = np.array([0xFFF, 0x005, 0, 0x801, 0xA5A], np.uint32)
    packed, src = dm.DeliveryModel().deliver(chunks, masks, 0)
    want = dm.slot_walk(chunks, masks)
    assert packed.shape == want.shape and (packed == want).all()
    assert src.tolist() == [f * PER + j for f in range(5) for j in range(PER) if (int(masks[f]) >> j) & 1]


def test_first_occurrence_wins():
    h = [0x89, 1, 2, 3, 0, 7]
    chunks = crafted(3, {(0, 5): h, (1, 0): h, (2, 11): h}, seed=2)
    masks = np.array([0xFFF, 0xFFF, 0xFFF], np.uint32)
    packed, src = dm.DeliveryModel().deliver(chunks, masks, dm.DEDUP)
    assert 5 in src and PER not in src and 2 * PER + 11 not in src and len(src) == 36 - 2
    assert (packed[src.tolist().index(5)] == chunks[0, 5]).all()          # the first one's payload, not a later one's
    masks[0] &= ~np.uint32(1 << 5)                                          # the first occurrence not delivered: the second is now the first
    _, src = dm.DeliveryModel().deliver(chunks, masks, dm.DEDUP)
    assert 5 not in src and PER in src and 2 * PER + 11 not in src


@pytest.mark.parametrize("byte", range(6))
def test_headers_one_byte_apart_are_kept_apart(byte):
    base = [0x91, 0x22, 0x33, 0x44, 0x55, 0x66]
    other = list(base)
    other[byte] ^= 0x01
    chunks = crafted(1, {(0, 0): base, (0, 1): other, (0, 2): base, (0, 3): other}, seed=3)
    _, src = dm.DeliveryModel().deliver(chunks, np.array([0xF], np.uint32), dm.DEDUP | dm.DROP_EMPTY)
    assert src.tolist() == [0, 1]


def test_drop_empty_comes_before_dedup():
    chunks = crafted(2, {(0, 0): [0] * 6, (0, 1): [0] * 6, (0, 2): [0x80, 0, 0, 0, 0, 0], (0, 3): [0x80, 0, 0, 0, 0, 0],
                         (1, 0): [0x7F, 0, 0, 0, 9, 9], (1, 1): [0, 0, 0, 1, 0, 0]}, seed=4)
    masks = np.array([0xF, 0x3], np.uint32)
    m = dm.DeliveryModel()
    _, src = m.deliver(chunks, masks, dm.DEDUP | dm.DROP_EMPTY | dm.REMEMBER)
    assert src.tolist() == [2, PER + 1]           # size bit 0x80 alone is a size; an encode id alone is not
    assert m.stats()[0] == 2                      # dropped empties are never remembered
    _, src = dm.DeliveryModel().deliver(chunks, masks, dm.DEDUP)
    assert src.tolist() == [0, 2, PER, PER + 1]   # without DROP_EMPTY the empty header is a header like any other
    _, src = dm.DeliveryModel().deliver(chunks, masks, dm.DROP_EMPTY)
    assert src.tolist() == [2, 3, PER + 1]


def test_remember_across_calls_and_reset():
    a = crafted(2, {}, seed=5)
    b = crafted(2, {}, seed=6)
    b[0, 3, :6] = a[1, 7, :6]
    b[1, 0, :6] = a[0, 0, :6]
    full = np.array([0xFFF, 0xFFF], np.uint32)
    m = dm.DeliveryModel()
    assert m.stats() == (0, 0, False)
    _, s1 = m.deliver(a, full, dm.REMEMBER | dm.DROP_EMPTY)
    assert len(s1) == 24 and m.stats() == (24, 1 << 20, False)
    _, s2 = m.deliver(b, full, dm.REMEMBER | dm.DROP_EMPTY)
    assert s2.tolist() == [i for i in range(24) if i not in (3, PER)] and m.stats()[0] == 46
    _, s3 = m.deliver(b, full, dm.DEDUP | dm.DROP_EMPTY)          # a call without REMEMBER neither asks nor tells
    assert len(s3) == 24 and m.stats()[0] == 46
    m.reset()
    _, s4 = m.deliver(b, full, dm.REMEMBER | dm.DROP_EMPTY)
    assert len(s4) == 24 and m.stats() == (24, 1 << 20, False)


def test_overflow_remembers_nothing_and_loses_nothing():
    m = dm.DeliveryModel()
    m.reset(4)                                    # 16 entries: at most 8 headers
    a = crafted(1, {}, seed=7)
    _, s = m.deliver(a, np.array([0x1F], np.uint32), dm.REMEMBER)
    assert len(s) == 5 and m.stats() == (5, 16, False)
    _, s = m.deliver(a, np.array([0x1FF], np.uint32), dm.REMEMBER)            # 4 new ones: 9 > 8
    assert s.tolist() == [5, 6, 7, 8] and m.stats() == (5, 16, True)          # the remembered ones are still dropped
    _, s = m.deliver(a, np.array([0x0E0], np.uint32), dm.REMEMBER)            # 3 new ones fit: 8
    assert s.tolist() == [5, 6, 7] and m.stats() == (8, 16, True)             # sticky
    b = crafted(1, {(0, 11): a[0, 2, :6]}, seed=8)
    _, s = m.deliver(b, np.array([0xFFF], np.uint32), dm.REMEMBER)            # more than 8 new headers in one call
    assert s.tolist() == list(range(11)) and m.stats() == (8, 16, True)       # all delivered, none remembered
    m.reset(4)
    assert m.stats() == (0, 16, False)
    _, s = m.deliver(b, np.array([0xFFF], np.uint32), dm.REMEMBER)
    assert len(s) == 12 and m.stats() == (0, 16, True)


def test_null_context_is_refused_before_any_device_work():
    """every delivery entry point checks its arguments before it touches the device: without a context there is nothing to run on"""
    from libcimbar_amd import decoder
    lib = decoder.load_library()
    buf = np.zeros(PER * CS, np.uint8)
    mask = np.zeros(1, np.uint32)
    src = np.zeros(PER, np.int32)
    count = ctypes.c_int32(-7)
    rc = lib.cimbar_hip_deliver_chunks(None, buf.ctypes.data, mask.ctypes.data, 1, decoder.MEM_HOST, 0, buf.ctypes.data, src.ctypes.data,
                                       ctypes.addressof(count), decoder.MEM_HOST, None)
    assert rc == -1 and count.value == -7
    assert lib.cimbar_hip_delivery_reset(None, 0) == -1
    a, b, c = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int(-7)
    assert lib.cimbar_hip_delivery_stats(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert (a.value, b.value, c.value) == (-7, -7, -7)
    assert (decoder.DELIVER_DEDUP, decoder.DELIVER_REMEMBER, decoder.DELIVER_DROP_EMPTY) == (dm.DEDUP, dm.REMEMBER, dm.DROP_EMPTY)
