"""A plain-Python restatement of the closing schedule of multi-capture decoding across calls (include/cimbar_hip.h,
cimbar_hip_decode_batch_combined_stream; csrc/combine.hip.inc "the stream calls"), written from the rule rather than from the kernels.

StreamModel(min_agree_permille, max_group) carries between calls only what the device carries: the symbols and colours of the open group's
members (at most max_group - 1 of them) and where each came from.

    call(symbols, colors, usable=None, flush=False) -> (groups_out (n,) int32, closed, gsizes)
        groups_out[k]  the call-local id of capture k's group if it closes in this call, GROUP_OPEN if it stays open, -1 if unusable
        closed         the groups this call closes, in order: each a list of (call number, index in that call) pairs
        gsizes         their member counts

run(calls, flushes, min_agree_permille, max_group) -> the per-call results of a whole sequence, calls = [(symbols, colors, usable), ...]
"""
import numpy as np

from tests import combine_model as CM

GROUP_OPEN = -2


class StreamModel:
    def __init__(self, min_agree_permille=0, max_group=0):
        self.min_agree, self.max_group = CM.resolve(min_agree_permille, max_group)
        self.open = []          # the carried members: (symbols row, colours row, (call, index))
        self.calls = 0

    def _joins(self, sym, col):
        """does a usable capture with these cells go on with the open group (which has room by construction)?"""
        if not self.open:
            return False
        ps, pc, _ = self.open[-1]
        a = int(CM.agree(np.stack([ps, sym]), np.stack([pc, col]))[0])
        return not (a * 1000 < self.min_agree * len(sym))

    def call(self, symbols, colors, usable=None, flush=False):
        n = len(symbols)
        usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
        if n == 0 and not flush:
            raise ValueError("n == 0 without a flush")
        out = np.full(n, -1, np.int32)
        closed = []

        def close():
            if self.open:
                gid = len(closed)
                closed.append([src for _, _, src in self.open])
                for _, _, (c, k) in self.open:
                    if c == self.calls:
                        out[k] = gid
                self.open = []

        for k in range(n):
            if not usable[k]:
                close()
                continue
            sym, col = np.asarray(symbols[k]), np.asarray(colors[k])
            if not self._joins(sym, col):
                close()
            self.open.append((sym, col, (self.calls, k)))
            if len(self.open) >= self.max_group:
                close()
        if flush:
            close()
        for _, _, (c, k) in self.open:
            if c == self.calls:
                out[k] = GROUP_OPEN
        assert len(self.open) <= self.max_group - 1
        self.calls += 1
        return out, closed, [len(g) for g in closed]


def run(calls, flushes, min_agree_permille=0, max_group=0):
    model = StreamModel(min_agree_permille, max_group)
    return [model.call(s, c, u, flush=f) for (s, c, u), f in zip(calls, flushes)]
