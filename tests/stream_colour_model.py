"""The colour vote in the stream calls (cimbar_hip_set_stream_colour_vote) restated in plain Python from the rule in include/cimbar_hip.h.

The model is combine_stream_model.StreamModel -- which decides what closes when -- plus, per carried member, what the device carries of it: the
per-capture results the group decode reads (symbols, colours, positions, bit plane, mask, chunks) and ONE FULL ROW OF WEIGHTS,
w = colour_erasure_model.margins(...) + 1 over every cell, taken while the member's frame and matrix are at hand. A carried member has no frame
and no matrix any more (`carried` drops them), so a closed group's vote can only come from the rows. Closed groups go through
group_colour_model.vote / decode_group.

    one_shot(mode, runs, ...)            the plain vote-on call over all captures: combine_model.group_captures' groups, margins from the frames
    StreamColourModel(mode, ...).call()  the same captures a few per call
Both return per closed group (members, gmask, gchunks, colour, gm).
"""
import functools

import numpy as np

from libcimbar_amd import geometry
from tests import colour_erasure_model as CE
from tests import combine_model as CM
from tests import combine_stream_model as SM
from tests import group_colour_cases as GC
from tests import group_colour_model as GM
from tests import symbol_erasure_cases as SC

CARRIED_KEYS = ("mask", "chunks", "symbols", "colours", "positions", "plane")
CUTS = ((1,) * 12, (3, 9), (5, 7), (2, 3, 4, 3))


def weights(run):
    """the weight row of one capture of symbol_erasure_cases.oracle_run's output (with its frame under "frame")"""
    return (CE.margins(CE.cell_means(run["frame"], run["positions"]), run["ccm"]).astype(np.int64) + 1).astype(np.uint32)


def carried(run):
    """what the carry keeps of a member: no frame, no matrix"""
    rec = {k: run[k] for k in CARRIED_KEYS}
    rec["weights"] = run["weights"] if "weights" in run else weights(run)
    return rec


_DECODED = {}


def decode_members(mode, recs, colour_margin=0):
    """one closed group from its members' records (each with a weight row) -> (gmask, gchunks, colour, gm). decode_group is a pure function of
    its inputs and costs seconds, so equal inputs are decoded once."""
    geo = geometry.for_mode(mode)
    cells, _, disputed = SC.combine_inputs(mode, recs, list(range(len(recs))))
    cols = np.stack([r["colours"] for r in recs])
    vc, gm, _ = GM.vote(cols, np.stack([r["weights"].astype(np.int64) - 1 for r in recs]))
    masks = [int(r["mask"]) for r in recs]
    chunks = [np.asarray(r["chunks"], np.uint8) for r in recs]
    key = (mode, colour_margin, cells.tobytes(), vc.tobytes(), gm.tobytes(), tuple(masks), tuple(c.tobytes() for c in chunks), disputed)
    if key not in _DECODED:
        _DECODED[key] = GM.decode_group(geo, cells & 15, vc, gm, masks, chunks, disputed, colour_margin=colour_margin)[:2]
    m, c = _DECODED[key]
    return m, c, vc, gm


def one_shot(mode, runs, min_agree_permille=0, max_group=0, colour_margin=0):
    """-> (groups (n,), [(members, gmask, gchunks, colour, gm)]) of the plain vote-on call over the captures"""
    groups = CM.group_captures([r["symbols"] for r in runs], [r["colours"] for r in runs], None, min_agree_permille, max_group)
    out = []
    for g in range(CM.n_groups(groups)):
        mem = CM.members(groups, g)
        recs = [dict(runs[k], weights=weights(runs[k])) for k in mem]      # the margins from the frames, as the plain call computes them
        out.append((mem,) + decode_members(mode, recs, colour_margin))
    return groups, out


class StreamColourModel:
    def __init__(self, mode, min_agree_permille=0, max_group=0, colour_margin=0):
        self.mode, self.colour_margin = mode, colour_margin
        self.walk = SM.StreamModel(min_agree_permille, max_group)
        self.carry = {}                      # (call, index) -> carried(run) of the open group's members

    def call(self, runs, flush=False):
        """runs: this call's captures (oracle_run dicts with "frame") -> (groups_out, [(sources, gmask, gchunks, colour, gm)] of the groups it closes)"""
        this = self.walk.calls
        out, closed, _ = self.walk.call([r["symbols"] for r in runs], [r["colours"] for r in runs], flush=flush)
        results = []
        for srcs in closed:
            recs = [self.carry[s] if s[0] != this else carried(runs[s[1]]) for s in srcs]
            results.append((srcs,) + decode_members(self.mode, recs, self.colour_margin))
        # the open group becomes the carry: carried members keep their rows, the call's own get theirs now
        self.carry = {s: (self.carry[s] if s[0] != this else carried(runs[s[1]])) for _, _, s in self.walk.open}
        return out, results


def run_cut(mode, runs, cut, **kw):
    """the captures cut into calls of `cut` captures, the last one flushed -> the closed groups in order, sources as indices into `runs`"""
    assert sum(cut) == len(runs)
    model = StreamColourModel(mode, **kw)
    starts = np.concatenate([[0], np.cumsum(cut)])
    closed = []
    for c, n in enumerate(cut):
        _, res = model.call(runs[starts[c]:starts[c] + n], flush=c == len(cut) - 1)
        for srcs, m, ch, vc, gm in res:
            closed.append(([int(starts[sc] + k) for sc, k in srcs], m, ch, vc, gm))
    assert not model.carry
    return closed


@functools.lru_cache(maxsize=None)
def pair_runs(mode):
    """group_colour_cases.pair_set(mode) through the oracle -> (runs with frames, payload)"""
    caps, payload, _ = GC.pair_set(mode)
    runs = SC.oracle_run(mode, caps)
    for r, fr in zip(runs, caps):
        r["frame"] = fr
    return runs, payload
