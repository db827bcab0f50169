"""Device time of tear skipping (cimbar_hip_set_once_tear_skip), mode 68, 1024 captures per call already in device memory, device outputs.

(a) clean   runs of three copies of a clean frame, no torn capture: the once-call enqueues k_repeat_tear and the tear forms of the two list
            kernels and nothing else it did not before. Timed: the setting off and on (axis 0), and -- with --parent-lib, a build of the
            parent commit -- two contexts on that library, so that off-against-on can be held against the parent's own back-to-back spread.
(b) torn    256 x [A, A + noise 40, A shifted (2, 1), cut(A, the next frame, "midcell")]: a run of three and a torn capture per displayed
            frame. Timed: the once-call with the setting off and on, and decode_batch on the same captures. Reported with the roles and the
            complete frames each delivers. The call's last capture is torn and has no successor, so it is decoded either way.
(c) whole   (b) with the last capture replaced by the next frame whole: the setting off and on.
(d) clean   (c) with [A, A, A] for the run of three: no representative takes the flood path, only the torn captures would.
The cases of a set alternate within every repetition; medians and min / max of the per-call times (device events around the call, the
once-call's read-backs included). Prints one JSON line; --out writes it to a file as well.

    python tools/once_tear_bench.py [--reps 20] [--parent-lib path/to/libcimbar_hip.so] [--out profiles/once_tear_bench.json]
    python tools/once_tear_bench.py --trace off|on|plain|off_c|on_c|off_d|on_d   # (_c, _d: sets c, d)
                                                              # set (b), one call of that case and nothing else, nothing timed: for
                                                              # rocprofv3 --kernel-trace --stats -- python tools/once_tear_bench.py --trace on
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
from tests import frames as F  # noqa: E402
from tests import stitch_cases as SC  # noqa: E402

MODE, N = 68, 1024


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


def torn_stream(dec, dev, last_clean=False, clean_repeats=False):
    """(captures (N, H, W, 3) on the device, payload (N / 4 + 1, FRAME_BYTES)); last_clean: the call's last capture is the next frame whole
    instead of the torn one (a torn capture at the end of a call has no successor to be held against and is decoded); clean_repeats: the
    run of three is [A, A, A]"""
    shown = N // 4
    payload = framegen.synth_payload(shown + 1, seed=47, mode=MODE).numpy().reshape(shown + 1, -1)
    clean = dec.encode_batch(payload)
    p = SC.tear_pixels(MODE, 0, "midcell")[0]
    out = torch.empty((N, *dec.geo.FRAME_SHAPE), dtype=torch.uint8, device=dev)
    for i in range(shown):
        A = clean[i]
        four = np.stack([A, A if clean_repeats else F.add_noise(A, 40, i), A if clean_repeats else F.shift(A, 2, 1), SC.cut(A, clean[i + 1], 0, p)])
        out[4 * i:4 * i + 4] = torch.from_numpy(four).to(dev)
    if last_clean:
        out[N - 1] = torch.from_numpy(clean[shown]).to(dev)
    return out, payload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libcimbar_hip.so built from the parent commit (set a)")
    ap.add_argument("--trace", default=None, choices=("off", "on", "plain", "off_c", "on_c", "off_d", "on_d"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    off, on = D.HipDecoder(0, MODE), D.HipDecoder(0, MODE)
    on.set_once_tear_skip(0)
    geo = off.geo
    mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)

    class Out:
        def __init__(self):
            self.chunks, self.masks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)
            self.runs, self.roles, self.n_runs = mk(N, torch.int32), mk(N, torch.int32), mk(1, torch.int32)
            self.rchunks, self.rmasks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)

    def once(dec, fr, o):
        return lambda: dec.decode_batch_once_device(fr.data_ptr(), N, o.chunks.data_ptr(), o.masks.data_ptr(), o.runs.data_ptr(), o.roles.data_ptr(),
                                                    o.rchunks.data_ptr(), o.rmasks.data_ptr(), o.n_runs.data_ptr(), stream=stream)

    def plain(dec, fr, o):
        return lambda: dec.decode_batch_device(fr.data_ptr(), N, o.chunks.data_ptr(), o.masks.data_ptr(), stream=stream)

    if a.trace:
        fr, _ = torn_stream(off, dev, a.trace[-2:] in ("_c", "_d"), a.trace.endswith("_d"))
        o = Out()
        call = {"off": once(off, fr, o), "on": once(on, fr, o), "plain": plain(off, fr, o)}[a.trace.split("_")[0]]
        call()
        torch.cuda.synchronize(dev)
        print(json.dumps({"trace": a.trace, "calls": 1, "roles": np.bincount(o.roles.cpu().numpy() + 1, minlength=5).tolist()}))
        return

    res = {"mode": MODE, "captures": N, "reps": a.reps}

    # (a) clean runs of three
    shown = (N + 2) // 3
    payload = framegen.synth_payload(shown, seed=31, mode=MODE).numpy().reshape(shown, -1)
    clean = torch.from_numpy(off.encode_batch(payload)).to(dev)[torch.arange(N, device=dev) // 3]
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
          "on_minus_off_us": round((med["on"] - med["off"]) * 1000, 1),
          "complete_runs_off": int((outs["off"].rmasks.cpu().numpy().view(np.uint32) == geo.FULL_MASK).sum()),
          "complete_runs_on": int((outs["on"].rmasks.cpu().numpy().view(np.uint32) == geo.FULL_MASK).sum()),
          "same_outputs": bool(all(torch.equal(getattr(outs["off"], k), getattr(outs["on"], k)) for k in ("chunks", "masks", "runs", "roles", "rchunks", "rmasks"))),
          "candidates": int((on.tap_once_tear(N)[:, 0] >= 0).sum())}
    if parents:
        both = t["parent_1"] + t["parent_2"]
        ca["parent_spread_ms"] = [round(min(both), 4), round(max(both), 4)]
        ca["parent_medians_ms"] = sorted([med["parent_1"], med["parent_2"]])
        ca["on_inside_the_parents_spread"] = bool(min(both) <= med["on"] <= max(both))
        ca["off_inside_the_parents_spread"] = bool(min(both) <= med["off"] <= max(both))
        ca["on_minus_parent_median_us"] = round((med["on"] - statistics.median(both)) * 1000, 1)
    res["clean_runs_of_three"] = ca
    for p in parents:
        p.close()
    del clean

    # (b) a run of three and a torn capture per displayed frame
    fr, want = torn_stream(off, dev)
    o_off, o_on, o_pl = Out(), Out(), Out()
    pl = D.HipDecoder(0, MODE)
    t = timed({"once_off": once(off, fr, o_off), "once_on": once(on, fr, o_on), "decode_batch": plain(pl, fr, o_pl)}, a.reps, dev)
    sb = summary(t)
    cb = {"times": sb}
    for name, o in (("once_off", o_off), ("once_on", o_on)):
        nr = int(o.n_runs.item())
        rm = o.rmasks.cpu().numpy().view(np.uint32)[:nr]
        rc = o.rchunks.cpu().numpy()[:nr]
        runs = o.runs.cpu().numpy()
        shows = np.zeros(nr, np.int64)
        shows[runs[np.arange(N) % 4 == 0]] = np.arange(N // 4)             # the displayed frame of every run that holds a clean capture
        full = rm == geo.FULL_MASK
        cb[name] = {"runs": nr, "complete_frames": int(full.sum()), "complete_frames_are_the_payload": bool((rc[full] == want[shows[full]]).all()),
                    "roles": dict(zip(("unusable", "skipped", "representative", "fallback", "torn"), np.bincount(o.roles.cpu().numpy() + 1, minlength=5).tolist()))}
    pm = o_pl.masks.cpu().numpy().view(np.uint32)
    cb["decode_batch"] = {"complete_captures": int((pm == geo.FULL_MASK).sum())}
    cb["same_complete_frames"] = bool(torch.equal(o_off.runs, o_on.runs) and np.array_equal(o_off.rmasks.cpu().numpy() == np.int32(geo.FULL_MASK), o_on.rmasks.cpu().numpy() == np.int32(geo.FULL_MASK)))
    cb["candidates"] = int((on.tap_once_tear(N)[:, 0] >= 0).sum())
    cb["on_median_below_off_min"] = bool(sb["once_on"]["median_ms"] < sb["once_off"]["min_ms"])
    cb["saved_ms"] = round(sb["once_off"]["median_ms"] - sb["once_on"]["median_ms"], 4)
    res["torn_every_fourth"] = cb

    # (c) the same, but the call ends on a whole frame; (d) and the repeats are clean copies, so that only the torn captures take the flood
    for key, kw in (("torn_every_fourth_last_capture_whole", dict(last_clean=True)),
                    ("clean_repeats_torn_every_fourth_last_capture_whole", dict(last_clean=True, clean_repeats=True))):
        del fr
        fr, want = torn_stream(off, dev, **kw)
        t = timed({"once_off": once(off, fr, o_off), "once_on": once(on, fr, o_on)}, a.reps, dev)
        sc = summary(t)
        cc = {"times": sc}
        for name, o in (("once_off", o_off), ("once_on", o_on)):
            nr = int(o.n_runs.item())
            rm = o.rmasks.cpu().numpy().view(np.uint32)[:nr]
            cc[name] = {"runs": nr, "complete_frames": int((rm == geo.FULL_MASK).sum()),
                        "roles": dict(zip(("unusable", "skipped", "representative", "fallback", "torn"), np.bincount(o.roles.cpu().numpy() + 1, minlength=5).tolist()))}
        cc["on_median_below_off_min"] = bool(sc["once_on"]["median_ms"] < sc["once_off"]["min_ms"])
        cc["saved_ms"] = round(sc["once_off"]["median_ms"] - sc["once_on"]["median_ms"], 4)
        res[key] = cc
    for d in (off, on, pl):
        d.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
