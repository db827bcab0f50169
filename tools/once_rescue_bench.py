"""Device time of the run rescue (cimbar_hip_set_once_rescue), mode 68, 256 captures per call already in device memory, and what it delivers.

(a) clean   runs of three copies of a clean frame (85 displayed frames and one capture of an 86th). No representative is incomplete, so the
            once-call enqueues the same launches with the setting on as with it off. Timed: the setting off and on, and -- with
            --parent-lib, a build of the parent commit -- two contexts on that library, so that off-against-on can be held against the
            parent's own back-to-back spread on the same box.
(b) pairs   128 disjoint-damage pairs (tests/once_rescue_model.pairs: the disc pairs of three frames in turn; neither capture of a pair
            decodes completely, the two together do). Timed: the once-call with min_agree_permille 500 and the rescue on, the same with it off,
            and decode_batch_combined (min_agree_permille 250, as the combine tests group these captures). Reported with the complete
            frames and the chunks each delivers.
The cases of a set alternate within every repetition; medians and min / max of the per-call times (device events around the call, the
once-call's read-backs included). Prints one JSON line; --out writes it to a file as well.

    python tools/once_rescue_bench.py [--reps 20] [--parent-lib path/to/libcimbar_hip.so] [--out profiles/once_rescue_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libcimbar_amd import decoder as D  # noqa: E402
from libcimbar_amd import framegen  # noqa: E402
from tests import group_walk_cases as GW  # noqa: E402
from tests import once_rescue_model as OM  # noqa: E402

MODE, N = 68, 256


def timed(calls, reps, dev):
    """every call once as a warm-up, then `reps` rounds of all of them in turn -> per-call times in ms"""
    for f in calls.values():
        f()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize(dev)
            times[k].append(t0.elapsed_time(t1))
    return times


def summary(times):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libcimbar_hip.so built from the parent commit (case a)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    off, on = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    on.set_once_rescue(True)
    geo = off.geo
    mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)

    class Out:
        def __init__(self):
            self.chunks, self.masks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)
            self.runs, self.roles, self.n_runs = mk(N, torch.int32), mk(N, torch.int32), mk(1, torch.int32)
            self.rchunks, self.rmasks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)

    def once(dec, fr, o, **kw):
        return lambda: dec.decode_batch_once_device(fr.data_ptr(), N, o.chunks.data_ptr(), o.masks.data_ptr(), o.runs.data_ptr(), o.roles.data_ptr(),
                                                    o.rchunks.data_ptr(), o.rmasks.data_ptr(), o.n_runs.data_ptr(), stream=stream, **kw)

    pop = lambda m: int(sum(bin(int(x)).count("1") for x in m))
    res = {"mode": MODE, "captures": N, "reps": a.reps}

    # (a) clean runs of three
    shown = (N + 2) // 3
    payload = framegen.synth_payload(shown, seed=31, mode=MODE).numpy().reshape(shown, -1)
    clean = torch.from_numpy(off.encode_batch(payload)[np.arange(N) // 3]).to(dev)
    outs = {k: Out() for k in ("off", "on", "parent_1", "parent_2")}
    calls = {"off": once(off, clean, outs["off"]), "on": once(on, clean, outs["on"])}
    parents = []
    if a.parent_lib:
        parents = [D.HipDecoder(0, MODE, lib_path=a.parent_lib), D.HipDecoder(0, MODE, lib_path=a.parent_lib)]
        calls["parent_1"], calls["parent_2"] = once(parents[0], clean, outs["parent_1"]), once(parents[1], clean, outs["parent_2"])
    t = timed(calls, a.reps, dev)
    sa = summary(t)
    med = {k: v["median_ms"] for k, v in sa.items()}
    ca = {"times": sa, "runs": int(outs["on"].n_runs.item()), "on_over_off": round(med["on"] / med["off"], 4),
          "complete_runs_off": int((outs["off"].rmasks.cpu().numpy().view(np.uint32) == geo.FULL_MASK).sum()),
          "complete_runs_on": int((outs["on"].rmasks.cpu().numpy().view(np.uint32) == geo.FULL_MASK).sum()),
          "same_outputs": bool(torch.equal(outs["off"].rchunks, outs["on"].rchunks) and torch.equal(outs["off"].rmasks, outs["on"].rmasks)),
          "rescue_tried": int((on.tap_once_rescue(N) != -1).sum())}
    if parents:
        ca["parent_2_over_parent_1"] = round(med["parent_2"] / med["parent_1"], 4)
        ca["off_over_parent_1"] = round(med["off"] / med["parent_1"], 4)
        ca["on_over_parent_1"] = round(med["on"] / med["parent_1"], 4)
        lo, hi = min(med["parent_1"], med["parent_2"]), max(med["parent_1"], med["parent_2"])
        ca["off_and_on_inside_the_parents_spread"] = bool(all(min(t["parent_1"] + t["parent_2"]) <= med[k] <= max(t["parent_1"] + t["parent_2"]) for k in ("off", "on")))
        ca["parent_medians_ms"] = [lo, hi]
    res["clean_runs_of_three"] = ca
    for p in parents:
        p.close()
    del clean

    # (b) 128 disjoint-damage pairs
    frames, want = OM.pairs(MODE, N // 2)
    fr = torch.from_numpy(frames.copy()).to(dev)       # (the cached captures are read-only)
    o_on, o_off, o_cb = Out(), Out(), Out()
    kw = dict(min_agree_permille=OM.MIN_AGREE, color_correction=0)
    comb = D.HipDecoder(0, MODE)
    calls = {"once_rescue": once(on, fr, o_on, **kw), "once_plain": once(off, fr, o_off, **kw),
             "combined": lambda: comb.decode_batch_combined_device(fr.data_ptr(), N, o_cb.chunks.data_ptr(), o_cb.masks.data_ptr(), o_cb.runs.data_ptr(),
                                                                   o_cb.rchunks.data_ptr(), o_cb.rmasks.data_ptr(), o_cb.n_runs.data_ptr(),
                                                                   min_agree_permille=GW.AGREE_3, color_correction=0, stream=stream)}
    t = timed(calls, a.reps, dev)
    sb = summary(t)
    cb = {"times": sb}
    for name, o in (("once_rescue", o_on), ("once_plain", o_off), ("combined", o_cb)):
        nr = int(o.n_runs.item())
        rm = o.rmasks.cpu().numpy().view(np.uint32)[:nr]
        rc = o.rchunks.cpu().numpy()[:nr]
        full = rm == geo.FULL_MASK
        genuine = bool(nr == N // 2 and (rc[full] == want[full]).all())
        cb[name] = {"frames_reported": nr, "complete_frames": int(full.sum()), "chunks_delivered": pop(rm), "complete_frames_are_the_payload": genuine}
    cb["rescue_tried"] = int((on.tap_once_rescue(N) != -1).sum())
    r, c = sb["once_rescue"]["median_ms"], sb["combined"]["median_ms"]
    cb["once_rescue_over_combined"] = round(r / c, 4)
    cb["faster"] = "once_rescue" if r < c else "combined"
    res["disjoint_damage_pairs"] = cb
    for d in (off, on, comb):
        d.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
