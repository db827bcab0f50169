"""CPU: the errors-and-erasures Reed-Solomon fixture (tests/golden/rs_erasures.json) and its restatement (tests/erasure_model.py).

- The file is self-consistent: every code the modes use is there, every family named in its generator is present, the restatement
  reproduces every recorded return value, message and acceptance status, the blocks built inside the correction budget decode to a
  codeword, and e > p always fails.
- The restatement is checked for the property erasures exist for: 2 * errors + erasures <= p decodes.
- With the reference build, libcorrect itself reproduces the file, with a fresh decoder object per block and with one reused object.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import erasure_model, rs_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_erasures.json")
FAMILIES = {"within", "budget", "ends", "clean", "padding", "overload", "over"}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _rows(code):
    for c in code["cases"]:
        yield c, np.frombuffer(bytes.fromhex(c["block"]), np.uint8), c["erasures"]


def test_golden_covers_every_code(golden):
    assert sorted((c["n"], c["parity"]) for c in golden["codes"]) == [(155, 30), (168, 33), (179, 36)]
    for code in golden["codes"]:
        fams = {c["family"] for c in code["cases"]}
        assert fams == FAMILIES, fams
        n, p = code["n"], code["parity"]
        counts = {len(c["erasures"]) for c in code["cases"] if c["family"] == "within"}
        assert counts == set(range(p + 1))
        ends = [c for c in code["cases"] if c["family"] == "ends"]
        assert all(0 in c["erasures"] and n - 1 in c["erasures"] for c in ends)
        assert code["reused_object_differs"] == 0
        # every status occurs: accepted, libcorrect failures, and raw successes the acceptance check rejects
        assert {c["status"] for c in code["cases"]} == {-1, 0, 1}


@pytest.mark.parametrize("n,p", [(155, 30), (179, 36), (168, 33)])
def test_model_reproduces_golden(golden, n, p):
    code = next(c for c in golden["codes"] if c["n"] == n)
    for c, block, er in _rows(code):
        assert len(block) == n and all(0 <= x < n for x in er)
        rc, msg, word, in_pad = erasure_model.decode(block, er, p)
        assert rc == c["rc"], (c["family"], len(er))
        if rc > 0:
            assert bytes(msg).hex() == c["msg"]
            assert (word[:n - p] == msg).all()
        assert erasure_model.status(rc, word, in_pad, p) == c["status"]
        if c["family"] == "over":
            assert len(er) > p and rc == -1 and c["status"] == -1
        if c["promised"]:
            assert c["status"] == 1 and not rs_cases.syndromes(word, p).any()
        if c["status"] == 1:
            assert not rs_cases.syndromes(word, p).any() and not in_pad


@pytest.mark.parametrize("n,p", [(155, 30), (179, 36), (168, 33)])
def test_model_decodes_within_budget(n, p):
    """A check of the restatement itself, not of the product: 2t + e <= p decodes to the sent message, whether or not the erased bytes are
    wrong; errors-only decoding (e = 0) stops at t = p // 2. The device's counterpart is test_gpu_rs_erasures.py's
    test_rs_erasures_recovers_twice_the_errors."""
    g = np.random.default_rng(n)
    k = n - p
    for e in (0, 1, p // 3, p // 2, p - 3, p - 1, p):
        t = (p - e) // 2
        msg = g.integers(0, 256, (1, k), dtype=np.uint8)
        c = rs_cases.encode(msg, p)[0]
        pos = g.permutation(n)
        bad = c.copy()
        hit = np.concatenate([pos[: e // 2], pos[e:e + t]]).astype(np.int64)
        bad[hit] ^= g.integers(1, 256, len(hit), dtype=np.uint8)
        rc, out, word, in_pad = erasure_model.decode(bad, pos[:e], p)
        assert rc == k and (out == msg[0]).all() and (word == c).all() and not in_pad
        assert erasure_model.status(rc, word, in_pad, p) == 1
    # p erased bytes, all wrong, and no error elsewhere: twice what errors-only decoding corrects
    c = rs_cases.encode(g.integers(0, 256, (1, k), dtype=np.uint8), p)[0]
    pos = g.permutation(n)[:p]
    bad = c.copy()
    bad[pos] ^= g.integers(1, 256, p, dtype=np.uint8)
    assert erasure_model.decode(bad, [], p)[0] == -1 or not (erasure_model.decode(bad, [], p)[2] == c).all()
    rc, out, word, _ = erasure_model.decode(bad, pos, p)
    assert rc == k and (word == c).all()


def _libcorrect(ref):
    L = ref
    L.correct_reed_solomon_create.argtypes = [ctypes.c_uint16, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_size_t]
    L.correct_reed_solomon_create.restype = ctypes.c_void_p
    L.correct_reed_solomon_destroy.argtypes = [ctypes.c_void_p]
    L.correct_reed_solomon_destroy.restype = None
    L.correct_reed_solomon_decode_with_erasures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                            ctypes.c_void_p]
    L.correct_reed_solomon_decode_with_erasures.restype = ctypes.c_ssize_t
    return L


def test_libcorrect_reproduces_golden(ref, golden):
    if not hasattr(ref, "correct_reed_solomon_decode_with_erasures"):
        pytest.skip("the reference build does not export libcorrect")
    L = _libcorrect(ref)
    for code in golden["codes"]:
        n, p = code["n"], code["parity"]
        shared = L.correct_reed_solomon_create(0x187, 1, 1, p)
        try:
            for c, block, er in _rows(code):
                blk = np.ascontiguousarray(block)
                era = np.array(er if er else [0], np.uint8)
                for rs in (None, shared):
                    own = L.correct_reed_solomon_create(0x187, 1, 1, p) if rs is None else rs
                    msg = blk[:n - p].copy()
                    rc = L.correct_reed_solomon_decode_with_erasures(own, blk.ctypes.data, n, era.ctypes.data, len(er), msg.ctypes.data)
                    if rs is None:
                        L.correct_reed_solomon_destroy(own)
                    assert rc == c["rc"], (n, c["family"], len(er))
                    if rc > 0:
                        assert bytes(msg).hex() == c["msg"]
        finally:
            L.correct_reed_solomon_destroy(shared)
