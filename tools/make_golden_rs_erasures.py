"""Writes tests/golden/rs_erasures.json: errors-and-erasures Reed-Solomon cases for every RS code the modes use -- RS(155,125) (modes 68, 4
and 8), RS(179,143) (67) and RS(168,135) (66) -- with libcorrect's own answer (correct_reed_solomon_decode_with_erasures out of the
reference build, oracle/_ref/libcimbar_ref.so, which exports it) and the acceptance status of tests/erasure_model.py.

Families per code (n, p):
  within      e = 0 .. p erasures, some on bytes that are correct, and (p - e) // 2 errors elsewhere: decodes to the sent message
  budget      2t + e = p - 1, p, p + 1, p + 2 (t errors outside e corrupted erasures), several e each
  ends        erasures on the first and the last byte of the block (both corrupted) with errors elsewhere
  clean       erasures only on correct bytes, (p - e) // 2 errors elsewhere
  padding     blocks whose long codeword has non-zero bytes in the shortened code's padding, with erasures: libcorrect "corrects" there
  overload    far more errors than the budget: libcorrect fails or miscorrects
  over        e > p: libcorrect returns -1 before decoding
Every block is decoded with a fresh correct_reed_solomon object. The tool also decodes all of them with one reused object and records in
the file whether that changed any result.

Run where the reference build exists: python tools/make_golden_rs_erasures.py
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import erasure_model, rs_cases  # noqa: E402

CODES = ((155, 30), (179, 36), (168, 33))
OUT = os.path.join(ROOT, "tests", "golden", "rs_erasures.json")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libcimbar_ref.so")


def libcorrect(path=REF_SO):
    L = ctypes.CDLL(path)
    L.correct_reed_solomon_create.argtypes = [ctypes.c_uint16, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_size_t]
    L.correct_reed_solomon_create.restype = ctypes.c_void_p
    L.correct_reed_solomon_destroy.argtypes = [ctypes.c_void_p]
    L.correct_reed_solomon_destroy.restype = None
    L.correct_reed_solomon_decode_with_erasures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                            ctypes.c_void_p]
    L.correct_reed_solomon_decode_with_erasures.restype = ctypes.c_ssize_t
    return L


def lc_decode(L, rs, block, erasures, parity):
    """(rc, msg) of correct_reed_solomon_decode_with_erasures; rs None: a fresh object (the reference's ReedSolomon wrapper's parameters,
    ReedSolomon.h:23-27: primitive polynomial 0x187, first consecutive root 1, root gap 1)"""
    own = rs is None
    if own:
        rs = L.correct_reed_solomon_create(0x187, 1, 1, parity)
    blk = np.ascontiguousarray(block, np.uint8)
    er = np.ascontiguousarray(erasures, np.uint8) if len(erasures) else np.zeros(1, np.uint8)
    msg = blk[:len(blk) - parity].copy()     # libcorrect leaves the buffer alone where it fails: the received bytes, as the device writes
    rc = L.correct_reed_solomon_decode_with_erasures(rs, blk.ctypes.data, len(blk), er.ctypes.data, len(erasures), msg.ctypes.data)
    if own:
        L.correct_reed_solomon_destroy(rs)
    return int(rc), msg


def _corrupt(g, block, pos):
    out = block.copy()
    pos = np.asarray(pos, np.int64)
    out[pos] ^= g.integers(1, 256, len(pos), dtype=np.uint8)
    return out


def cases(g, n, p):
    k = n - p
    enc = lambda: rs_cases.encode(g.integers(0, 256, (1, k), dtype=np.uint8), p)[0]   # noqa: E731
    out = []
    for e in range(p + 1):                                            # within
        c = enc()
        pos = g.permutation(n)
        er, rest = pos[:e], pos[e:]
        hit = er[: (e + 1) // 2]                                      # about half the erasures on bytes that are actually wrong
        t = (p - e) // 2
        out.append(("within", _corrupt(g, c, np.concatenate([hit, rest[:t]])), er, c[:k], True))
    for target in (p - 1, p, p + 1, p + 2):                           # budget
        for e in sorted({x for x in (1, 2, p // 4, p // 2, p - 4, p - 2, p - 1, p) if 0 < x <= p}):
            if (target - e) < 0 or (target - e) % 2:
                continue
            t = (target - e) // 2
            c = enc()
            pos = g.permutation(n)
            er = pos[:e]
            out.append(("budget", _corrupt(g, c, np.concatenate([er, pos[e:e + t]])), er, c[:k], target <= p))
    for e, t in ((2, 0), (2, (p - 2) // 2), (p - 2, 1), (p, 0)):      # ends
        c = enc()
        mid = g.permutation(np.arange(1, n - 1))
        er = np.concatenate([[0, n - 1], mid[: e - 2]])
        out.append(("ends", _corrupt(g, c, np.concatenate([er, mid[e - 2:e - 2 + t]])), er, c[:k], True))
    for e in (1, p // 3, p // 2, p):                                  # clean: erased bytes all correct
        c = enc()
        pos = g.permutation(n)
        out.append(("clean", _corrupt(g, c, pos[e:e + (p - e) // 2]), pos[:e], c[:k], True))
    pad = 255 - n
    for e in (1, 4, p // 2, p - 2):                                   # padding
        for j in (1, 3):
            long_msg = np.zeros(255 - p, np.uint8)
            long_msg[g.choice(pad, j, replace=False)] = g.integers(1, 256, j, dtype=np.uint8)
            long_msg[pad:] = g.integers(0, 256, k, dtype=np.uint8)
            long = rs_cases.encode(long_msg[None], p)[0]
            pos = g.permutation(n)
            out.append(("padding", _corrupt(g, long[pad:], pos[:e // 2]), pos[:e], None, False))
    for _ in range(24):                                               # overload
        e = int(g.integers(1, p + 1))
        c = enc()
        pos = g.permutation(n)
        t = int(g.integers((p - e) // 2 + 2, (p - e) // 2 + 12))
        out.append(("overload", _corrupt(g, c, np.concatenate([pos[:e], pos[e:e + t]])), pos[:e], None, False))
    for e in (p + 1, p + 5, n):                                       # over
        c = enc()
        out.append(("over", _corrupt(g, c, g.choice(n, 2, replace=False)), g.permutation(n)[:e], None, False))
    return out


def main():
    L = libcorrect()
    g = np.random.default_rng(20261015)
    doc = {"generator": "tools/make_golden_rs_erasures.py", "decoder": "libcorrect correct_reed_solomon_decode_with_erasures, a fresh object per block",
           "codes": []}
    for n, p in CODES:
        rows, reuse_diff = [], 0
        shared = L.correct_reed_solomon_create(0x187, 1, 1, p)
        counts = {}
        for fam, block, er, want, promised in cases(g, n, p):
            rc, msg = lc_decode(L, None, block, er, p)
            rc2, msg2 = lc_decode(L, shared, block, er, p)
            reuse_diff += int(rc2 != rc or (rc > 0 and not (msg2 == msg).all()))
            mrc, mmsg, word, in_pad = erasure_model.decode(block, er, p)
            assert mrc == rc and (rc < 0 or (mmsg == msg).all()), (n, fam, rc, mrc)
            st = erasure_model.status(rc, word, in_pad, p)
            if promised:
                assert rc > 0 and (msg == want).all() and st == 1, (n, fam, len(er), rc, st)
            counts.setdefault(fam, [0, 0, 0])[st + 1] += 1
            rows.append({"family": fam, "block": bytes(block).hex(), "erasures": [int(x) for x in er], "rc": rc,
                         "msg": bytes(msg).hex() if rc > 0 else None, "status": st, "promised": bool(promised)})
        L.correct_reed_solomon_destroy(shared)
        print(f"RS({n},{n - p}): {len(rows)} blocks; status -1/0/1 per family: {counts}; reused object changed {reuse_diff}")
        doc["codes"].append({"n": n, "parity": p, "reused_object_differs": reuse_diff, "cases": rows})
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
