"""numpy restatement of chunk delivery (include/cimbar_hip.h, cimbar_hip_deliver_chunks / _delivery_reset / _delivery_stats): what the device
must reproduce byte for byte. Plain loops and a Python set -- no table, no hash: the rules, not the mechanism.

  candidates   the (frame, slot) pairs whose mask bit is set, in ascending frame * chunks_per_frame + slot
  DROP_EMPTY   first: a candidate whose header says file size 0 -- (b0 & 0x80) == 0 and b1 == b2 == b3 == 0 -- is dropped and never remembered
  DEDUP        the first candidate of the call with those six header bytes is kept
  REMEMBER     implies DEDUP; a candidate whose header an earlier REMEMBER call delivered is dropped; the call's delivered headers are
               remembered when remembered + delivered <= capacity / 2, else NONE of them is and the sticky overflow flag is set
"""
import numpy as np

DEDUP, REMEMBER, DROP_EMPTY = 1, 2, 4
DEFAULT_CAPACITY_LOG2 = 20


def header_key(chunk):
    """the 48-bit header of a chunk as an int (FountainMetadata::md_size = 6 bytes, big-endian here only to make an int of them)"""
    return int.from_bytes(bytes(bytearray(chunk[:6])), "big")


def is_empty(chunk):
    """FountainMetadata::file_size() == 0"""
    return (int(chunk[0]) & 0x80) == 0 and int(chunk[1]) == 0 and int(chunk[2]) == 0 and int(chunk[3]) == 0


def slot_walk(chunks, masks):
    """the host loop the receive shim runs per frame (for j in per: if mask & (1 << j): memcpy), concatenated over the batch"""
    n, per, cs = chunks.shape
    out = [chunks[f, j] for f in range(n) for j in range(per) if (int(masks[f]) >> j) & 1]
    return np.stack(out) if out else np.zeros((0, cs), np.uint8)


class DeliveryModel:
    """one context's delivery state"""

    def __init__(self):
        self.capacity = 0            # no table until the first REMEMBER call or reset()
        self.seen = set()
        self.overflowed = False

    def reset(self, capacity_log2=0):
        if capacity_log2 != 0 and not 4 <= capacity_log2 <= 24:
            raise ValueError("capacity_log2 must be 0 or 4 .. 24")
        self.capacity = 1 << (capacity_log2 or DEFAULT_CAPACITY_LOG2)
        self.seen = set()
        self.overflowed = False

    def stats(self):
        return len(self.seen), self.capacity, self.overflowed

    def deliver(self, chunks, masks, flags):
        """chunks (n, per, cs) uint8, masks (n,) -> (packed (count, cs) uint8, src (count,) int32)"""
        if flags & ~(DEDUP | REMEMBER | DROP_EMPTY):
            raise ValueError("unknown flag bits")
        if flags & REMEMBER:
            flags |= DEDUP
            if not self.capacity:
                self.reset(0)
        chunks = np.asarray(chunks, np.uint8)
        n, per, cs = chunks.shape
        mine = set()
        kept = []
        for f in range(n):
            for j in range(per):
                if not (int(masks[f]) >> j) & 1:
                    continue
                c = chunks[f, j]
                if (flags & DROP_EMPTY) and is_empty(c):
                    continue
                if flags & DEDUP:
                    k = header_key(c)
                    if k in mine:
                        continue
                    mine.add(k)
                    if (flags & REMEMBER) and k in self.seen:
                        continue
                kept.append(f * per + j)
        if flags & REMEMBER:
            new = {header_key(chunks.reshape(n * per, cs)[i]) for i in kept}
            if len(self.seen) + len(new) <= self.capacity // 2:
                self.seen |= new
            else:
                self.overflowed = True
        src = np.array(kept, np.int32).reshape(-1)
        packed = chunks.reshape(n * per, cs)[src] if len(kept) else np.zeros((0, cs), np.uint8)
        return np.ascontiguousarray(packed), src
