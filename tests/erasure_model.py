"""A plain-Python restatement of libcorrect's errors-and-erasures decode (correct_reed_solomon_decode_with_erasures, decode.c:381-508) and of
the acceptance check cimbar_hip_rs_decode_erasures adds to it. It writes the steps out the way libcorrect does: the 8-bit location remap,
the erasure locator prod (x + 1/X_i), the modified syndromes, Berlekamp-Massey over the remaining p - e, Chien over the error locator,
Forney over erasure locator * error locator with the original syndromes (fcr = 1), and field_div(x, 0) == 0. Where libcorrect's behaviour
is undefined (a locator order whose look-up rows it does not have) the block counts as failed, as on the device.

decode(block, erasures, parity) -> (rc, msg, word, in_pad):
  rc      libcorrect's return value: the message length, or -1
  msg     the n - p message bytes libcorrect writes (the received ones where rc is -1)
  word    the corrected n-byte block (only the message part of it is visible through libcorrect)
  in_pad  a root of the combined locator lies in the shortened code's zero padding (location >= n)
status(...) -> -1 / 0 / 1: what cimbar_hip_rs_decode_erasures reports per block.
"""
import numpy as np

from tests.rs_cases import EXP, LOG, syndromes

_EXP = [int(x) for x in EXP]
_LOG = [int(x) for x in LOG]


def _mul(a, b):
    return 0 if a == 0 or b == 0 else _EXP[_LOG[a] + _LOG[b]]


def _div(a, b):
    return 0 if a == 0 or b == 0 else _EXP[255 + _LOG[a] - _LOG[b]]


def _eval(coef, order, x):
    """sum_i coef[i] x^i, i <= order, x != 0"""
    res, acc, lx = 0, 0, _LOG[x] % 255
    for i in range(order + 1):
        if coef[i]:
            res ^= _EXP[_LOG[coef[i]] % 255 + acc]
        acc = (acc + lx) % 255
    return res


def decode(block, erasures, parity):
    block = [int(v) for v in block]
    n, k = len(block), len(block) - parity
    e = len(erasures)
    word = list(block)
    if e > parity:                                   # decode.c:392
        return -1, np.array(block[:k], np.uint8), np.array(word, np.uint8), False
    S = [int(v) for v in syndromes(block, parity)]
    if not any(S):
        return k, np.array(block[:k], np.uint8), np.array(word, np.uint8), False
    roots = [_div(1, _EXP[(n - 1 - int(p)) & 0xFF]) for p in erasures]     # decode.c:424 (block_length - (pos + pad + 1)), 226-235
    eloc = [1]
    if e:
        eloc = [roots[0], 1]
        for r in roots[1:]:                          # polynomial_init_from_roots: (x + r) * eloc
            eloc = [(eloc[i - 1] if i >= 1 else 0) ^ (_mul(r, eloc[i]) if i < len(eloc) else 0) for i in range(len(eloc) + 1)]
    mod = [0] * parity                               # eloc * S mod x^p
    for i, c in enumerate(eloc):
        for j in range(parity - i):
            mod[i + j] ^= _mul(c, S[j])
    T = mod[e:]
    # Berlekamp-Massey (decode.c:32-118)
    size = 2 * parity + 12
    loc, last = [0] * size, [0] * size
    loc[0] = last[0] = 1
    loc_order = last_order = numerrors = 0
    delay, last_disc = 1, 1
    for i in range(parity - e):
        disc = T[i]
        for j in range(1, numerrors + 1):
            disc ^= _mul(loc[j], T[i - j])
        if not disc:
            delay += 1
            continue
        if 2 * numerrors <= i:
            for j in range(last_order, -1, -1):
                if j + delay < size:
                    last[j + delay] = _div(_mul(last[j], disc), last_disc)
            for j in range(delay - 1, -1, -1):
                if j < size:
                    last[j] = 0
            for j in range(min(last_order + delay + 1, size)):
                loc[j], last[j] = loc[j] ^ last[j], loc[j]
            loc_order, last_order = last_order + delay, loc_order
            numerrors = i + 1 - numerrors
            last_disc, delay = disc, 1
            continue
        for j in range(last_order, -1, -1):
            if j + delay < size:
                loc[j + delay] ^= _div(_mul(last[j], disc), last_disc)
        loc_order = max(loc_order, last_order + delay)
        delay += 1
    order = loc_order
    fail = (-1, np.array(block[:k], np.uint8), np.array(word, np.uint8), False)
    if order >= parity or order + e > parity:       # past libcorrect's look-up rows: undefined there, a failure here
        return fail
    found = [x for x in range(1, 256) if _eval(loc, order, x) == 0]     # Chien (decode.c:122-145); element 0 is never a root
    if len(found) != order:
        return fail
    roots = roots + found
    total = e + order
    full = [0] * (total + 1)
    for i, c in enumerate(eloc):
        for j in range(order + 1):
            full[i + j] ^= _mul(c, loc[j])
    ev = [0] * parity
    for i in range(min(total, parity - 1) + 1):
        for j in range(parity - i):
            ev[i + j] ^= _mul(full[i], S[j])
    der = [full[i + 1] if i % 2 == 0 else 0 for i in range(total)]
    in_pad = False
    for x in roots:
        val = _div(_eval(ev, parity - 1, x), _eval(der, total - 1, x) if total >= 1 else 0)
        X = _div(1, x)
        where = 0 if X == 1 else _LOG[X]
        if where < n:
            word[n - 1 - where] ^= val
        else:
            in_pad = True
    return k, np.array(word[:k], np.uint8), np.array(word, np.uint8), in_pad


def status(rc, word, in_pad, parity):
    """cimbar_hip_rs_decode_erasures' per-block status: -1 libcorrect fails; 1 the corrected word is a codeword and nothing was located in
    the padding; 0 otherwise (libcorrect "succeeds" with a miscorrection)"""
    if rc < 0:
        return -1
    return 1 if not in_pad and not syndromes(word, parity).any() else 0
