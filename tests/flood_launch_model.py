"""Which launches of the exact flood replay (k_flood3) one decode call makes: a plain restatement of the host's rule (plan_chain() and
exact_launch() in libcimbar_amd/csrc/chainplan.hip.inc, which enqueue() in host.hip.inc issues), in the terms of
CIMBAR_HIP_TAP_FLOOD_LAUNCH. No GPU, no library: tests/test_flood_launch_model.py checks its invariants, tests/test_chain_plan.py holds the
host's plan against it on a CPU, tests/test_gpu_flood_shapes.py holds HipDecoder.tap_flood_launches() against it.

The rule. A = the spill areas a launch may use: FLOOD_GRID = 1024 for a batch that runs as one chain, 512 per stream of a split batch,
1024 / pipe_depth per pipelined set; A3 = A * 768 / 1024. A launch of m frames is

    dense (eight frames per CU)   where CIMBAR_HIP_FLOOD_DENSE=1, or it is unset and m > A:  grid min(m, 2 A dense_grid / 2048)
    three frames per CU           else where m <= A3:                                         grid m
    four frames per CU            else:                                                       grid min(m, A)

and a launch with grid < m hands the other frames out through counter pair `counter`. Launches that may be in flight together get their own
range of areas and their own counter: stream 0 / 1 of a split batch base 0 / 512 and counter 0 / 1, pipelined set k base k A and counter k.
The bases are in units of `scale` areas: 2 (the dense instance's workgroups per ordinary one) on a context that may launch the dense
instance at all (dense != 0), 1 where it never does -- one spacing for every instance, because a dense launch on one pipelined set and an
ordinary one on another may run side by side.
"""

FLOOD_GRID, FLOOD_GRID3, DENSE_PER = 1024, 768, 2
FLOOD_COUNTERS = 8          # counter pairs the context holds
MAX_RECORDS = 16            # what the tap keeps of one call
FIELDS = ("instance", "grid", "frames", "first_frame", "area0", "counter", "flags")
BATCH_FLAGS, VERIFY_REPLAY, FALLBACK_REPLAY = 0, 1, 2


def splits(n, entry="plain", tail_split=1, tail_parts=2, mostly_flood=False, timed=False):
    """does the chain behind the threshold pass run as tail_parts parts on two streams? Only the plain entry points split: a pipelined
    batch is one chain on its set's stream, the capture path (`capture`: scan + extract + decode, and every other caller that sets
    ChainArgs::no_split) asks for one chain, a timed batch is measured stage by stage; `mostly_flood` = more than a quarter of the batch
    before took a flood kernel (two half-size exact replays cost more than one)."""
    assert entry in ("plain", "pipelined", "capture")
    return entry == "plain" and not timed and bool(tail_split) and not mostly_flood and n >= 64 * tail_parts


def parts(n, P):
    """[(first frame, frames)] of the P parts of a split batch; part q runs on stream q & 1"""
    lo = [n * q // P for q in range(P + 1)]
    return [(lo[q], lo[q + 1] - lo[q]) for q in range(P)]


def areas(entry, split, pipe_depth):
    return FLOOD_GRID // pipe_depth if entry == "pipelined" else (FLOOD_GRID // 2 if split else FLOOD_GRID)


def scale(dense):
    return DENSE_PER if dense != 0 else 1


def one_launch(m, first_frame, A, area0, counter, dense, dense_grid, flags):
    A3 = A * FLOOD_GRID3 // FLOOD_GRID
    if dense > 0 or (dense < 0 and m > A):
        instance, grid = 8, min(m, DENSE_PER * A * dense_grid // (DENSE_PER * FLOOD_GRID))
    elif m <= A3:
        instance, grid = 3, m
    else:
        instance, grid = 4, min(m, A)
    return dict(instance=instance, grid=grid, frames=m, first_frame=first_frame, area0=area0, counter=counter, flags=flags)


def launches(n, entry="plain", pipe_depth=2, pipe_set=0, tail_split=1, tail_parts=2, mostly_flood=False, dense=-1, dense_grid=2048,
             verify=False, relaxed_fallback=None, wave=True, timed=False, with_lanes=False):
    """-> (records in issue order, areas_reserved) of one call of n frames; with_lanes: (records, areas_reserved, lanes), lanes[i] = the
    queue record i runs on -- ("set", k) for pipelined set k, ("stream", 0 / 1) for the caller's stream and the context's second one. Launches
    on one lane run one after the other; launches on different lanes may be in flight together.
    entry: "plain" (decode_batch and its kin), "pipelined" (set pipe_set of a pipeline pipe_depth deep) or "capture" (never split).
    dense / dense_grid: CIMBAR_HIP_FLOOD_DENSE (-1 = unset) / CIMBAR_HIP_FLOOD_DENSE_GRID. verify: CIMBAR_HIP_FLOOD_VERIFY (replays only
    where the batch-parallel pass runs at all: `wave`). relaxed_fallback: None = the relaxed flood is off; 0 / 1 = on, without / with the exact
    fallback -- the frames are then flooded in rounds, and the only exact launch for the batch's own flags is the fallback's."""
    split = splits(n, entry, tail_split, tail_parts, mostly_flood, timed)
    A = areas(entry, split, pipe_depth)
    sc = scale(dense)
    # what the context is asked to hold: up to the end of the LAST range that this kind of call may index
    off = sc * ((pipe_depth - 1) * A if entry == "pipelined" else (FLOOD_GRID // 2 if split else 0))
    dense_sized = dense > 0 or (dense < 0 and n > A)
    reserved = off + min(n, DENSE_PER * A if dense_sized else A)
    kinds = ([] if relaxed_fallback is not None else [BATCH_FLAGS]) + ([VERIFY_REPLAY] if verify and wave else []) \
        + ([FALLBACK_REPLAY] if relaxed_fallback else [])
    recs, lanes = [], []
    chain = parts(n, tail_parts) if split else [(0, n)]
    for q, (fa, m) in enumerate(chain):
        second = split and (q & 1)
        base = pipe_set * A if entry == "pipelined" else (FLOOD_GRID // 2 if second else 0)
        counter = pipe_set if entry == "pipelined" else (1 if second else 0)
        lane = ("set", pipe_set) if entry == "pipelined" else ("stream", 1 if second else 0)
        for kind in kinds:
            recs.append(one_launch(m, fa, A, sc * base, counter, dense, dense_grid, kind))
            lanes.append(lane)
    if with_lanes:
        return recs[:MAX_RECORDS], reserved, lanes[:MAX_RECORDS]
    return recs[:MAX_RECORDS], reserved


def has_hand_out(rec, A):
    """may this launch have fewer workgroups than frames? (the dense instance, and the four-per-CU one past its A workgroups)"""
    return rec["instance"] == 8 or (rec["instance"] == 4 and rec["frames"] > A)
