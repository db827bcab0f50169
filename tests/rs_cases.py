"""Reed-Solomon blocks at and past the correction limit, for any (block length n, parity p) a mode uses, and the renderer that puts a
frame's stream bytes back into cells. Shared by tests/test_oracle_vs_ref.py (the oracle against libcorrect) and tests/test_gpu_rs_fuzz.py (k_rs
against the oracle), so that both see the same blocks.

A case is (block, family, want): `block` the n received bytes, `want` the n - p message bytes a correct decoder must return -- or None where no
outcome is promised (more than t = p // 2 errors: libcorrect may fail or "succeed" with other bytes). The families:
  random      0 .. max errors at random positions
  boundary    t-1 .. t+2 errors at random positions, as a front burst, as a burst ending on the last byte (error location 0: the X == 1 alias),
              across the message/parity boundary, around bytes 63/64 and 127/128 and on the last byte of the third register (byte n - 1)
  zero        an all-zero codeword with errors only in the parity bytes; errors equal to the byte they hit (the received byte is 0)
  padding     the last n bytes of a length-255 codeword whose 255 - n leading bytes are not all zero, plus in-block errors: libcorrect
              corrects locations >= n that the shortened block does not have and drops them
  vanishing   a codeword of the parity-s code (s = p-5 .. p-1) read as a parity-p block: syndromes 0 .. s-1 vanish, syndrome s does not, so
              Berlekamp-Massey jumps to a locator of length s + 1 after s zero discrepancies, with a long `delay`
  vanishing+errors  the same with one or two byte errors added: the jump comes after a short locator, and the taps it adds above lane 31
              (p = 36) meet non-zero syndromes in the iterations after it -- the only blocks for which k_rs's discrepancy reduction needs lanes
              32 and up. (Such a locator has more than t taps, so the block fails whatever those lanes add: the outcome cannot tell the
              64-lane reduction from a 32-lane one. At p = 33 the terms above lane 31 are zero for every input.)
"""
import numpy as np
import torch

from libcimbar_amd import framegen

EXP, LOG = framegen._EXP, framegen._LOG       # GF(2^8), poly 0x187: the tables the encoder uses

FAMILIES = ("random", "boundary", "zero", "padding", "vanishing", "vanishing+errors")


def encode(msgs, parity):
    """(N, k) uint8 -> (N, k + parity) systematic codewords (framegen.rs_encode: libcorrect's encoder, pinned to the reference build)"""
    return framegen.rs_encode(torch.from_numpy(np.ascontiguousarray(msgs, dtype=np.uint8)), parity).numpy().copy()


def syndromes(block, count):
    """S_j = r(alpha^(j+1)), j < count, r(x) = sum_i block[n-1-i] x^i (libcorrect decode.c:12-28), in plain numpy"""
    r = np.asarray(block, np.int64)[::-1]
    nz = np.nonzero(r)[0]
    out = np.zeros(count, np.int64)
    for j in range(count):
        terms = EXP[(LOG[r[nz]] + (j + 1) * nz) % 255]
        out[j] = np.bitwise_xor.reduce(terms) if len(terms) else 0
    return out


def _corrupt(g, block, pos):
    bad = block.copy()
    pos = np.asarray(pos, np.int64)
    bad[pos] ^= g.integers(1, 256, len(pos), dtype=np.uint8)
    return bad


def random_cases(g, n, parity, count, max_errors):
    """`count` blocks with 0 .. max_errors errors each, at random positions"""
    k = n - parity
    enc = encode(g.integers(0, 256, (count, k), dtype=np.uint8), parity)
    out = []
    for c in range(count):
        ne = int(g.integers(0, max_errors + 1))
        out.append((_corrupt(g, enc[c], g.choice(n, ne, replace=False)), "random", enc[c, :k].copy() if ne <= parity // 2 else None))
    return out


def _placements(g, n, parity, ne):
    k = n - parity
    regs = [63, 64, 127, 128, n - 1, 62, 65, 126, 129, n - 2, 61, 66, 125, 130, n - 3, 60, 67, 124, 131, n - 4, 0, 1, 2, 3]
    yield "random", g.choice(n, ne, replace=False)
    yield "front", np.arange(ne)
    yield "tail", n - 1 - np.arange(ne)
    yield "msg/parity", (k - ne // 2 + np.arange(ne)) % n
    yield "around 64", 64 - ne // 2 + np.arange(ne)
    yield "around 128", 128 - ne // 2 + np.arange(ne)
    yield "register edges", np.array(regs[:ne])


def boundary_cases(g, n, parity):
    t, k = parity // 2, n - parity
    out = []
    for ne in (t - 1, t, t + 1, t + 2):
        for _, pos in _placements(g, n, parity, ne):
            assert len(set(pos.tolist())) == ne and pos.min() >= 0 and pos.max() < n
            enc = encode(g.integers(0, 256, (1, k), dtype=np.uint8), parity)[0]
            out.append((_corrupt(g, enc, pos), "boundary", enc[:k].copy() if ne <= t else None))
    return out


def zero_cases(g, n, parity):
    t, k = parity // 2, n - parity
    out = []
    for ne in (1, t - 1, t, t + 1):
        bad = _corrupt(g, np.zeros(n, np.uint8), k + g.choice(parity, ne, replace=False))       # all-zero codeword, parity bytes hit
        out.append((bad, "zero", np.zeros(k, np.uint8) if ne <= t else None))
    for ne in (1, t - 1, t, t + 1):
        enc = encode(g.integers(1, 256, (1, k), dtype=np.uint8), parity)[0]
        nonzero = np.nonzero(enc)[0]
        bad = enc.copy()
        bad[g.choice(nonzero, ne, replace=False)] = 0                                               # error value == the byte: received 0
        out.append((bad, "zero", enc[:k].copy() if ne <= t else None))
    return out


def padding_cases(g, n, parity):
    """(block, "padding", want): the long codeword's bytes [255 - n, 255 - n + k) are the message libcorrect must return"""
    t, k, pad = parity // 2, n - parity, 255 - n
    out = []
    for j, e in ((1, 0), (1, t - 1), (t // 2, t - t // 2), (t, 0), (2, 3), (t - 1, 1)):
        msg = np.zeros(255 - parity, np.uint8)
        msg[g.choice(pad, j, replace=False)] = g.integers(1, 256, j, dtype=np.uint8)
        msg[pad:] = g.integers(0, 256, k, dtype=np.uint8)
        long = encode(msg[None], parity)[0]
        assert np.count_nonzero(long[:pad]) == j
        out.append((_corrupt(g, long[pad:], g.choice(n, e, replace=False)), "padding", long[pad:pad + k].copy()))
    return out


def vanishing_cases(g, n, parity):
    out = []
    for s in range(parity - 5, parity):
        for extra in ((0,) if s == parity - 1 else (0, 1, 2)):
            while True:
                enc = encode(g.integers(0, 256, (1, n - s), dtype=np.uint8), s)[0]
                bad = _corrupt(g, enc, g.choice(n, extra, replace=False))
                S = syndromes(bad, s + 1)
                if extra or S[s] != 0:
                    break
            out.append((bad, "vanishing" if not extra else "vanishing+errors", None))
    return out


def vanishing_ok(block, parity):
    """the property a pure vanishing case was built with: for some s in p-5 .. p-1, S_0 .. S_(s-1) are zero and S_s is not"""
    S = syndromes(block, parity)
    lead = int(np.argmax(S != 0)) if S.any() else parity
    return parity - 5 <= lead < parity


def edge_cases(g, n, parity):
    return boundary_cases(g, n, parity) + zero_cases(g, n, parity) + padding_cases(g, n, parity) + vanishing_cases(g, n, parity)


def check_promise(case, parity, rc, out):
    """what the case was built to produce, whatever any implementation says: success with the sent message for <= t errors; the vanishing
    syndromes for a pure vanishing case"""
    block, family, want = case
    if family == "vanishing":
        assert vanishing_ok(block, parity), "vanishing: the leading syndromes are not what the case was built with"
    if want is not None:
        assert rc > 0 and (np.asarray(out) == want).all(), f"{family}: a correctable block was not decoded to the sent message (rc {rc})"


def blocks_to_tiles(synth, blocks):
    """stream bytes (F, BLOCKS * RS_BLOCK) uint8 -> tile index (colour * 16 + symbol) per linear cell, (F, NCELLS) int64: what the mode's
    encoder lays out (Encoder::encode_next: 4-bit symbol and 2-bit colour streams; encode_next_coupled in the legacy modes: the one stream read
    6 or 7 bits per cell, colour above symbol)"""
    g = synth.geo
    f = blocks.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(blocks).reshape(f, g.BLOCKS * g.RS_BLOCK).astype(np.int64))
    if g.LEGACY:
        cb = 4 + g.COLOR_BITS
        bits = ((b[:, :, None] >> torch.arange(7, -1, -1)) & 1).reshape(f, g.NCELLS, cb)
        stream = (bits * (2 ** torch.arange(cb - 1, -1, -1))).sum(dim=2)
    else:
        sym = b[:, :g.SYM_BLOCKS * g.RS_BLOCK]
        col = b[:, g.SYM_BLOCKS * g.RS_BLOCK:]
        sym_cells = torch.stack([sym >> 4, sym & 15], dim=2).reshape(f, g.NCELLS)
        col_cells = torch.stack([(col >> 6) & 3, (col >> 4) & 3, (col >> 2) & 3, col & 3], dim=2).reshape(f, g.NCELLS)
        stream = col_cells * 16 + sym_cells
    out = torch.empty((f, g.NCELLS), dtype=torch.int64)
    out[:, synth.stream_cell] = stream
    return out
