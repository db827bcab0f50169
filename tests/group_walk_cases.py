"""Inputs for the tests of the group walks (csrc/combine.hip.inc k_group_walk with groups_in == nullptr, k_group_walk_stream) past their
first step of 64 captures, and the damage helpers the combine tests share.

A batch is a list of RUNS. A run is r consecutive captures of one rendered frame: copies of it, or ("damaged") the two captures of a
disjoint-damage pair of it in turn, p0 p1 p0 p1 ... Consecutive runs show different frames (run i shows frame i % 3), so the rule
(tests/combine_model.group_captures) breaks between runs and nowhere else, and the cap (max_group) cuts inside a run.

WALK_CASES / STREAM_CASES / CAPTURE_* are the committed cases. tests/test_group_walk_cases.py vets them without a GPU -- every shape a
hand-over between two steps can get wrong is present, a lane-by-lane simulation of the kernels reproduces the rule on them, and the simulation with any
one carried variable forgotten does not; tests/test_gpu_group_walk.py runs them on the device.
"""
import numpy as np

N_FRAMES = 3           # distinct rendered frames
# per mille: below what two captures with a third of the frame damaged each share, 16 times what two different frames do (1 / 64 of the
# cells agree by chance). The pairs below damage a tenth of the frame each, so two captures of one run share far more than this.
AGREE_3 = 250


# ------------------------------------------------------------------------------------------------ damage (shared with the combine tests)
def disc(frame, cx, cy, r, kind, seed):
    h, w, _ = frame.shape
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * min(h, w)) ** 2
    if kind == "white":
        frame[d] = 255
    elif kind == "black":
        frame[d] = 0
    else:
        frame[d] = np.random.default_rng(seed).integers(0, 256, (int(d.sum()), 3), dtype=np.uint8)
    return frame


def band(frame, x0, x1, kind, seed):
    """a fill over columns [x0, x1) and rows [0.1, 0.9) of the frame (fractions; the corner anchors stay clean)"""
    h, w, _ = frame.shape
    ys, xs = slice(int(0.1 * h), int(0.9 * h)), slice(int(x0 * w), int(x1 * w))
    if kind == "white":
        frame[ys, xs] = 255
    elif kind == "black":
        frame[ys, xs] = 0
    else:
        frame[ys, xs] = np.random.default_rng(seed).integers(0, 256, frame[ys, xs].shape, dtype=np.uint8)
    return frame


# The interleave spreads each Reed-Solomon block over one half of the frame (top or bottom), so damage must reach both halves to cost a
# capture every chunk. Two captures: discs on the middle row, left and right; three: the thirds of the frame's width.
PLACES = [(0.30, 0.50), (0.70, 0.50)]
R = 0.19
KINDS = ("white", "black", "noise")


def damaged_group(frame, m, seed, kinds=KINDS):
    if m == 2:
        return [disc(frame.copy(), cx, cy, R, kinds[(seed + c) % len(kinds)], seed * 10 + c) for c, (cx, cy) in enumerate(PLACES)]
    return [band(frame.copy(), c / m, (c + 1) / m, kinds[(seed + c) % len(kinds)], seed * 10 + c) for c in range(m)]


# ------------------------------------------------------------------------------------------------ run lists
FILLER = ((1, False), (2, True), (3, False), (2, False), (5, False), (1, False), (4, True), (2, True), (6, False), (3, True))


class Runs:
    """a run list under construction: (length, damaged) per run, run i showing frame i % N_FRAMES"""

    def __init__(self):
        self.runs, self.n = [], 0

    def run(self, length, damaged=False):
        self.runs.append((int(length), bool(damaged)))
        self.n += length
        return self

    def until(self, pos):
        """short filler runs up to capture pos - 1: the next run starts at pos"""
        i = len(self.runs)
        while self.n < pos:
            length, damaged = FILLER[i % len(FILLER)]
            self.run(min(length, pos - self.n), damaged)
            i += 1
        assert self.n == pos
        return self


def expand(runs):
    """-> frame (n,), variant (n,), run (n,): the frame each capture shows, which rendering of it (0 the clean frame, 1 / 2 the members
    of its damaged pair) and the run it belongs to"""
    frame, variant, run = [], [], []
    for i, (length, damaged) in enumerate(runs):
        for r in range(length):
            frame.append(i % N_FRAMES)
            variant.append(1 + r % 2 if damaged else 0)
            run.append(i)
    return np.array(frame), np.array(variant), np.array(run)


def unique_index(runs):
    """the index of each capture in rendered()'s array of distinct captures"""
    frame, variant, _ = expand(runs)
    return frame * 3 + variant


def synthetic_cells(runs):
    """(symbols, colours) rows that stand for the captures in the rule and in the simulation: captures of one frame agree on every cell,
    captures of two frames on none"""
    frame, _, _ = expand(runs)
    sym = np.repeat(frame[:, None], 8, axis=1).astype(np.uint8)
    return sym, np.zeros_like(sym)


# straddles: a damaged run of 4 over 63|64 and over 127|128, a damaged run of 8 over 191|192 (one group at max_group 8)
RUNS_STRADDLE = Runs().until(62).run(4, True).until(126).run(4, True).until(188).run(8, True).until(200).runs
# a run of 75 from capture 61: step 64 .. 127 has no break in it, and where the cap cuts depends on the run's start (61 is no multiple of
# 3, 4 or 8; 64 no multiple of 3)
RUNS_LONG = Runs().until(61).run(75, True).until(140).runs
# a run ends at capture 63: the next group's head is lane 0 of the second step
RUNS_HEAD_64 = Runs().until(64).run(3, True).until(70).runs
# a group's head is lane 63 of the first step, its other members are in the second
RUNS_HEAD_63 = Runs().until(63).run(3, True).until(70).runs

RUN_LISTS = {"straddle": RUNS_STRADDLE, "long": RUNS_LONG, "head64": RUNS_HEAD_64, "head63": RUNS_HEAD_63}

# (run list, max_group as passed -- 0 is the default, 4): the plain combined calls
WALK_CASES = [("straddle", 0), ("straddle", 8), ("straddle", 3), ("long", 3), ("long", 1), ("long", 0), ("long", 8), ("head64", 0),
              ("head63", 3), ("head63", 0)]
# the straddling groups that must recover: (run list, max_group) -> first members
RECOVERING = {("straddle", 0): (62, 126), ("straddle", 8): (62, 126, 188)}

# the capture path: the straddle list as camera captures, blank (status <= 0) at 63, 64 and 127 and over 190 .. 193
CAPTURE_RUNS = RUNS_STRADDLE
CAPTURE_BLANKS = (63, 64, 127, 190, 191, 192, 193)
CAPTURE_SIZE = (1280, 720)
CAPTURE_QUAD = ((270, 20), (1010, 30), (260, 690), (1020, 680))       # (tests/test_gpu_stream_colour.py)
CAPTURE_CAPS = (0, 3)


def capture_usable(n=None):
    n = sum(r[0] for r in CAPTURE_RUNS) if n is None else n
    u = np.ones(n, bool)
    u[list(CAPTURE_BLANKS)] = False
    return u


# the stream calls: (run list, max_group, call sizes; 0 = a flush-only call). The last call of each is flushed.
# Found by a search over call sizes for the endings and carried counts that tests/test_group_walk_cases.py asserts of them.
STREAM_CASES = [("straddle", 3, (7, 64, 65, 62, 0, 2)), ("straddle", 3, (65, 3, 128, 4)), ("straddle", 3, (67, 127, 5, 1)),
                ("straddle", 8, (62, 131, 7)), ("straddle", 0, (5, 64, 131)), ("long", 3, (3, 62, 1, 64, 10))]
# the capture path of the stream calls, over CAPTURE_RUNS with CAPTURE_BLANKS
STREAM_CAPTURE_CASES = [("straddle", 0, (4, 64, 62, 63, 3, 1, 3)), ("straddle", 0, (66, 127, 7)), ("straddle", 3, (4, 67, 129))]


# ------------------------------------------------------------------------------------------------ rendering (the GPU tests)
def rendered(mode, kinds=KINDS):
    """-> (captures (3 * N_FRAMES, H, W, 3) indexed by unique_index(), payload (N_FRAMES, bytes)): the frames and the disjoint-damage pairs
    of test_recovery_from_disjoint_damage[m = 2], which that test shows to recover"""
    from libcimbar_amd import framegen
    payload = framegen.synth_payload(N_FRAMES, seed=300 + mode + 2, mode=mode)
    frames = framegen.FrameSynth("cpu", mode).frames_from_payload(payload).numpy().copy()
    out = []
    for k in range(N_FRAMES):
        out += [frames[k]] + damaged_group(frames[k], 2, k, kinds=kinds)
    return np.stack(out), payload.numpy().reshape(N_FRAMES, -1)
