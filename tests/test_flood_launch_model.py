"""CPU: the launch rule of the exact flood replay as tests/flood_launch_model.py restates it -- the sizing of the spill buffer against the
areas the launches index, the ranges and counters of launches in flight together, the hand-out, the instance boundaries -- swept over
every batch size up to 2 200 frames (split batches: also around 4 096 and 8 192, where a part first passes 512 frames), every pipeline
depth, split count, dense setting and dense grid. A disagreement between the two halves of the
host's rule (what ensure_flood_areas is asked for / what the launches index) shows here without a GPU."""
import itertools
import os
import re

import pytest

from tests import flood_launch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = range(1, 2201)
# ... and where the parts of a split batch pass 512 frames one after the other, so that a dense launch on one stream runs beside an ordinary
# one on the other -- in either order: with eight parts 4 101 frames put 513 on stream 0 (part 4) and 512 on stream 1 (part 5)
NS_SPLIT = list(NS) + list(range(4090, 4140)) + list(range(8180, 8230))
DENSE = (-1, 0, 1)
GRIDS = (2048, 1792, 8)          # CIMBAR_HIP_FLOOD_DENSE_GRID: the default, seven per CU, and the tests' tiny one


def extent(rec):
    return rec["area0"], rec["area0"] + rec["grid"]


def check_call(recs, reserved, A, dense_grid, lanes):
    """what holds for every call by itself"""
    assert len(lanes) == len(recs)
    for r in recs:
        lo, hi = extent(r)
        assert 0 <= lo and hi <= reserved, (r, reserved)                                    # (every instance indexes area0 + block)
        assert 1 <= r["grid"] <= r["frames"] and 0 <= r["counter"] < M.FLOOD_COUNTERS
        assert r["grid"] == r["frames"] or M.has_hand_out(r, A), r
        cap = {3: A * 768 // 1024, 4: A, 8: 2 * A * dense_grid // 2048}[r["instance"]]
        assert r["grid"] == min(r["frames"], cap), r
    # parts on the two streams of a split batch may run side by side
    for a, la in zip(recs, lanes):
        for b, lb in zip(recs, lanes):
            assert (la != lb) == (a["counter"] != b["counter"]), (a, la, b, lb)         # its own counter pair per lane, and only per lane
            if la != lb:
                (al, ah), (bl, bh) = extent(a), extent(b)
                assert ah <= bl or bh <= al, (a, b)
    # ... and the parts cover the batch once per kind
    for kind in {r["flags"] for r in recs}:
        mine = [r for r in recs if r["flags"] == kind]
        assert [r["first_frame"] for r in mine] == [sum(x["frames"] for x in mine[:k]) for k in range(len(mine))]


def test_the_header_and_the_python_side_name_the_tap():
    from libcimbar_amd import decoder as D
    header = open(os.path.join(ROOT, "include", "cimbar_hip.h")).read()
    assert re.search(r"\bCIMBAR_HIP_TAP_FLOOD_LAUNCH\s*=\s*34\b", header) and D.TAP_FLOOD_LAUNCH == 34
    assert D.FLOOD_LAUNCH_FIELDS == M.FIELDS and D.FLOOD_LAUNCH_MAX == M.MAX_RECORDS
    assert hasattr(D.HipDecoder, "tap_flood_launches")
    numbers = [int(v) for v in re.findall(r"\bCIMBAR_HIP_TAP_\w+\s*=\s*(\d+)", header)]
    assert sorted(numbers) == list(range(len(numbers))), "tap numbers are dense and unique"


@pytest.mark.parametrize("dense", DENSE)
@pytest.mark.parametrize("depth", (2, 3, 4))
def test_pipelined_sets_never_share_an_area_or_a_counter(depth, dense):
    A = 1024 // depth
    for grid in GRIDS:
        lo, hi = [10 ** 9] * depth, [0] * depth                    # the extent of everything set k may index, over every batch size
        for k in range(depth):
            for n in NS:
                recs, reserved, lanes = M.launches(n, "pipelined", pipe_depth=depth, pipe_set=k, dense=dense, dense_grid=grid, with_lanes=True)
                assert len(recs) == 1 and recs[0]["counter"] == k and recs[0]["frames"] == n and recs[0]["first_frame"] == 0
                assert lanes == [("set", k)]
                check_call(recs, reserved, A, grid, lanes)
                # (batches of different sizes may follow one another through the pipeline: the reservation must not depend on the set)
                assert reserved == M.launches(n, "pipelined", pipe_depth=depth, pipe_set=0, dense=dense, dense_grid=grid)[1]
                a, b = extent(recs[0])
                lo[k], hi[k] = min(lo[k], a), max(hi[k], b)
        for k in range(depth - 1):
            assert hi[k] <= lo[k + 1], f"depth {depth}, dense {dense}, grid {grid}: set {k} reaches {hi[k]}, set {k + 1} starts at {lo[k + 1]}"


def test_a_dense_set_beside_an_ordinary_one():
    """the case the sweep above found in the rule as it was (bases k A for the ordinary instances, 2 k A for the dense one): depth 4, default
    settings, 300 frames on set 0 (dense, areas [0, 300)) while 200 frames replay on set 1 (four per CU, then areas [256, 456))"""
    a, _ = M.launches(300, "pipelined", pipe_depth=4, pipe_set=0)
    b, _ = M.launches(200, "pipelined", pipe_depth=4, pipe_set=1)
    assert (a[0]["instance"], b[0]["instance"]) == (8, 4)
    assert extent(a[0]) == (0, 300) and extent(b[0]) == (512, 712)


@pytest.mark.parametrize("dense", DENSE)
@pytest.mark.parametrize("P", (2, 4, 8))
def test_plain_batches_split_and_unsplit(P, dense):
    mixed = set()                                      # (instance on stream 0, instance on stream 1) of launches within one call
    for n, mostly, grid in itertools.product(NS_SPLIT, (False, True), GRIDS):
        recs, reserved, lanes = M.launches(n, "plain", tail_parts=P, mostly_flood=mostly, dense=dense, dense_grid=grid, with_lanes=True)
        split = n >= 64 * P and not mostly
        assert split == M.splits(n, "plain", 1, P, mostly)
        assert len(recs) == (P if split else 1) and sum(r["frames"] for r in recs) == n
        check_call(recs, reserved, 512 if split else 1024, grid, lanes)
        mixed |= {(a["instance"], b["instance"]) for a, la in zip(recs, lanes) for b, lb in zip(recs, lanes) if la < lb}
        if split:
            assert lanes == [("stream", q & 1) for q in range(P)]
            assert [r["counter"] for r in recs] == [q & 1 for q in range(P)]
            assert all(abs(r["frames"] - n / P) < 1 for r in recs)
            assert {r["area0"] for r in recs if r["counter"] == 0} == {0}
            assert {r["area0"] for r in recs if r["counter"] == 1} == {512 * M.scale(dense)}
        else:
            assert recs[0]["area0"] == 0 and recs[0]["counter"] == 0 and lanes == [("stream", 0)]
    if dense < 0:
        # the sweep did put a dense launch on stream 1 beside an ordinary one on stream 0 and, where the parts allow it (only with eight: a part
        # on stream 0 larger than one on stream 1), the other way round -- the case the doubled base of stream 1 is there for
        assert (4, 8) in mixed and ((8, 4) in mixed) == (P == 8), (P, mixed)
    # what never splits: the capture path, a timed batch, CIMBAR_HIP_TAIL_SPLIT=0
    for n in NS:
        for kw in (dict(entry="capture"), dict(timed=True), dict(tail_split=0)):
            recs, reserved, lanes = M.launches(n, **{"entry": "plain", "tail_parts": P, "dense": dense, "with_lanes": True, **kw})
            assert len(recs) == 1 and recs[0]["frames"] == n
            check_call(recs, reserved, 1024, 2048, lanes)


@pytest.mark.parametrize("A,kw", [(1024, dict(entry="capture")), (512, dict(entry="pipelined", pipe_depth=2, pipe_set=1)),
                                  (341, dict(entry="pipelined", pipe_depth=3, pipe_set=2)), (256, dict(entry="pipelined", pipe_depth=4, pipe_set=3))])
def test_instance_boundaries(A, kw):
    A3 = A * 768 // 1024
    one = lambda n, **more: M.launches(n, **kw, **more)[0][0]
    for dense in (-1, 0):
        assert (one(A3, dense=dense)["instance"], one(A3, dense=dense)["grid"]) == (3, A3)
        assert (one(A3 + 1, dense=dense)["instance"], one(A3 + 1, dense=dense)["grid"]) == (4, A3 + 1)
        assert (one(A, dense=dense)["instance"], one(A, dense=dense)["grid"]) == (4, A)
    assert (one(A + 1)["instance"], one(A + 1)["grid"]) == (8, A + 1)
    assert (one(A + 1, dense=0)["instance"], one(A + 1, dense=0)["grid"]) == (4, A)
    assert (one(2 * A + 5)["instance"], one(2 * A + 5)["grid"]) == (8, 2 * A)
    assert (one(1, dense=1)["instance"], one(A + 1, dense=1, dense_grid=8)["grid"]) == (8, 8 * A // 1024)


def test_a_split_batch_at_its_instance_boundaries():
    # 2 x 384 = three per CU on both streams; one frame more and stream 1 takes the four-per-CU instance
    assert [r["instance"] for r in M.launches(768)[0]] == [3, 3]
    assert [(r["instance"], r["frames"]) for r in M.launches(769)[0]] == [(3, 384), (4, 385)]
    assert [(r["instance"], r["grid"]) for r in M.launches(1024)[0]] == [(4, 512), (4, 512)]
    assert [(r["instance"], r["frames"]) for r in M.launches(1025)[0]] == [(4, 512), (8, 513)]
    assert [(r["instance"], r["grid"]) for r in M.launches(1025, dense=0)[0]] == [(4, 512), (4, 512)]


def test_verify_and_fallback_replays_are_launches_of_their_own():
    base, reserved = M.launches(300)
    for kw, kinds in ((dict(verify=True), [0, 1]), (dict(verify=True, wave=False), [0]), (dict(relaxed_fallback=0), []),
                      (dict(relaxed_fallback=1), [2]), (dict(relaxed_fallback=1, verify=True), [1, 2])):
        recs, res = M.launches(300, **kw)
        assert res == reserved and [r["flags"] for r in recs] == kinds * 2
        for kind in kinds:
            assert [{**r, "flags": 0} for r in recs if r["flags"] == kind] == base
    assert len(M.launches(2048, tail_parts=8, verify=True, relaxed_fallback=1)[0]) == M.MAX_RECORDS
    assert len(M.launches(2048, tail_parts=8, verify=True)[0]) == M.MAX_RECORDS
