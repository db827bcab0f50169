"""CPU: the host's launch plan (libcimbar_amd/csrc/chainplan.hip.inc, plan_chain + exact_launch: what enqueue() issues) held against
tests/flood_launch_model.py -- the exact-replay records, their lanes and the spill areas reserved, at every boundary of the rule, for every
entry, pipeline depth and set, split setting, dense setting and relaxed-flood setting. The plan is plain C++: tools/chain_plan_shim.cpp puts it
behind a C symbol, g++ compiles that into a scratch directory, ctypes loads it. Lanes that can be in flight together must also get disjoint
spill areas, wave queues and counters by the planner's own figures."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import flood_launch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 63, 64, 127, 128, 129, 191, 192, 193, 255, 256, 257, 341, 342, 384, 385, 511, 512, 513, 768, 769, 1024, 1025, 2048, 2049, 4101)
ENTRIES = ("plain", "pipelined", "capture")
SETS = [(depth, k) for depth in (2, 3, 4) for k in range(depth)]
RELAXED = (None, 0, 1)           # off, on without fallback, on with fallback
FW_GRID = 512


class Plan:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        self.inp = np.zeros(17, np.int32)
        self.recs = np.zeros((M.MAX_RECORDS, 7), np.int32)
        self.lanes = np.zeros(M.MAX_RECORDS, np.int32)
        self.head = np.zeros(5, np.int32)
        self.lane_out = np.zeros((2, 5), np.int32)
        self.args = [x.ctypes.data_as(ctypes.c_void_p) for x in (self.inp, self.recs, self.lanes, self.head, self.lane_out)]
        self.lib.chain_plan.argtypes = [ctypes.c_void_p] * 5

    def __call__(self, n, entry, depth, k, tail_split, parts, mostly, timed, wave, verify, dense, grid, relaxed):
        pipe = entry == "pipelined"
        # (enqueue(): a pipelined batch is never timed; mostly_flood = more than a quarter of the batch before left the parallel path)
        self.inp[:] = (n, pipe, entry == "capture", timed and not pipe, 1 if mostly else 0, 2 if mostly else 0, 0, tail_split, parts, depth, k,
                       dense, grid, wave, verify, relaxed is not None, bool(relaxed))
        count = self.lib.chain_plan(*self.args)
        recs = [dict(zip(M.FIELDS, map(int, r))) for r in self.recs[:count]]
        lanes = [("set", k) if pipe else ("stream", int(l)) for l in self.lanes[:count]]
        return recs, int(self.head[1]), lanes


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("chainplan") / "libchain_plan.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "chain_plan_shim.cpp")], check=True)
    return Plan(so)


def test_the_constants_are_the_models(plan):
    out = np.zeros(6, np.int32)
    plan.lib.chain_plan_constants(out.ctypes.data_as(ctypes.c_void_p))
    assert tuple(out) == (M.FLOOD_GRID, M.FLOOD_GRID3, M.DENSE_PER, FW_GRID, M.FLOOD_COUNTERS, M.MAX_RECORDS)


def extent(rec):
    return rec["area0"], rec["area0"] + rec["grid"]


def disjoint(a, b):
    return a[1] <= b[0] or b[1] <= a[0]


@pytest.mark.parametrize("parts", (2, 4, 8))
@pytest.mark.parametrize("depth,k", SETS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_plan_is_the_models(plan, entry, depth, k, parts):
    rest = itertools.product(NS, (0, 1), (False, True), (False, True), (True, False), (False, True), (-1, 0, 1), (2048, 1792), RELAXED)
    for n, tail_split, mostly, timed, wave, verify, dense, grid, relaxed in rest:
        got = plan(n, entry, depth, k, tail_split, parts, mostly, timed, int(wave), int(verify), dense, grid, relaxed)
        want = M.launches(n, entry, pipe_depth=depth, pipe_set=k, tail_split=tail_split, tail_parts=parts, mostly_flood=mostly, dense=dense,
                          dense_grid=grid, verify=verify, relaxed_fallback=relaxed, wave=wave, timed=timed, with_lanes=True)
        case = (n, entry, depth, k, tail_split, parts, mostly, timed, wave, verify, dense, grid, relaxed)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (case, got, want)
        # the planner's own figures: what a lane's launches index lies inside what is reserved; lanes in flight together share nothing
        recs, reserved, lanes = got
        assert all(0 <= extent(r)[0] and extent(r)[1] <= reserved for r in recs), (case, recs, reserved)
        split = int(plan.head[2])
        assert split == M.splits(n, entry, tail_split, parts, mostly, timed)
        if split:
            (a, a0, w, w0, c), (b, b0, wb, wb0, cb) = (tuple(int(v) for v in row) for row in plan.lane_out)
            assert c != cb and 0 <= min(c, cb) and max(c, cb) < M.FLOOD_COUNTERS
            assert disjoint((w0, w0 + w), (wb0, wb0 + wb)) and max(w0 + w, wb0 + wb) <= FW_GRID, (case, plan.lane_out)
            for (r, lr), (s, ls) in itertools.combinations(zip(recs, lanes), 2):
                assert (lr != ls) == (r["counter"] != s["counter"]), (case, r, s)
                assert lr == ls or disjoint(extent(r), extent(s)), (case, r, s)


@pytest.mark.parametrize("dense", (-1, 0, 1))
@pytest.mark.parametrize("depth", (2, 3, 4))
def test_pipelined_sets_share_nothing(plan, depth, dense):
    """batches of any size may follow one another through the pipeline: whatever set k may index, over every n, ends where set k + 1 begins"""
    for grid, verify, relaxed in itertools.product((2048, 1792), (False, True), RELAXED):
        lo, hi, queues, counters = [10 ** 9] * depth, [0] * depth, [None] * depth, [None] * depth
        for k, n in itertools.product(range(depth), NS):
            reserved0 = plan(n, "pipelined", depth, 0, 1, 2, False, False, 1, int(verify), dense, grid, relaxed)[1]
            recs, reserved, _ = plan(n, "pipelined", depth, k, 1, 2, False, False, 1, int(verify), dense, grid, relaxed)
            assert reserved == reserved0                               # (the reservation must not depend on the set)
            _, _, w, w0, c = (int(v) for v in plan.lane_out[0])
            assert (queues[k], counters[k]) in ((None, None), ((w0, w0 + w), c))            # a set's shares do not depend on n
            queues[k], counters[k] = (w0, w0 + w), c
            for r in recs:
                assert r["counter"] == c and extent(r)[1] <= reserved
                lo[k], hi[k] = min(lo[k], extent(r)[0]), max(hi[k], extent(r)[1])
        assert len(set(counters)) == depth and all(0 <= c < M.FLOOD_COUNTERS for c in counters)
        assert all(hi[k] <= lo[k + 1] for k in range(depth - 1)), (depth, dense, grid, lo, hi)
        assert all(disjoint(a, b) for a, b in itertools.combinations(queues, 2)) and max(q[1] for q in queues) <= FW_GRID, queues
