"""Device time of tear salvage (cimbar_hip_set_once_tear_salvage), mode 68, 256 captures per call already in device memory, device outputs.
Every once-call context has the run rescue and tear skipping (axis 0, line_permille 650) on and calls with min_agree_permille 950;
"off" / "on" is tear salvage alone.

(a) clean   64 x [A, A, A, cut(A, the next frame, "bottom")]: clean runs of three with a torn capture after each. Every representative comes
            back complete, so every candidate is left undecoded and nothing is salvaged: the setting must cost nothing. Timed: off, on, and
            -- with --parent-lib, a build of the parent commit -- two contexts on that library (rescue and tear skipping on), so that off
            and on can be held against the parent's own back-to-back spread.
(b) wiped   64 x [wipe8(A_i), cut(A_i, A_i+1, "bottom"), A_i+1, A_i+1]: a damaged run of one, the torn capture that shows its damaged
            region clean, and a clean run of two. Timed: the once-call off and on, and decode_batch_combined on the same captures.
            Reported: the complete run rows (group rows) each delivers, how many distinct displayed frames those are, and whether every
            delivered chunk is the payload's.
The cases of a set alternate within every repetition; medians and min / max of the per-call times (device events around the call, the
once-call's read-backs included). Prints one JSON line; --out writes it to a file as well.

    python tools/once_salvage_bench.py [--reps 20] [--parent-lib path/to/libcimbar_hip.so] [--out profiles/once_salvage_bench.json]
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
from tests import repeat_skip_cases as RC  # noqa: E402
from tests import stitch_cases as SC  # noqa: E402

MODE, N, SHOWN = 68, 256, 64
MIN_AGREE, LINE = 950, 650


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


def context(lib_path=None, salvage=False):
    d = D.HipDecoder(0, MODE, lib_path=lib_path)
    d.set_once_rescue(True)
    d.set_once_tear_skip(0, LINE)
    if salvage:
        d.set_once_tear_salvage(True)
    return d


def captures(dec, dev, wiped):
    """(captures (N, H, W, 3) on the device, payload (SHOWN + 1, FRAME_BYTES), the displayed frame of every capture, -1 for a torn one)"""
    payload = framegen.synth_payload(SHOWN + 1, seed=53, mode=MODE).numpy().reshape(SHOWN + 1, -1)
    clean = dec.encode_batch(payload)
    p = SC.tear_pixels(MODE, 0, "bottom")[1]
    out = torch.empty((N, *dec.geo.FRAME_SHAPE), dtype=torch.uint8, device=dev)
    shows = np.zeros(N, np.int64)
    for i in range(SHOWN):
        A, B = clean[i], clean[i + 1]
        four = [RC.wipe8(MODE, A), SC.cut(A, B, 0, p), B, B] if wiped else [A, A, A, SC.cut(A, B, 0, p)]
        out[4 * i:4 * i + 4] = torch.from_numpy(np.stack(four)).to(dev)
        shows[4 * i:4 * i + 4] = [i, -1, i + 1, i + 1] if wiped else [i, i, i, -1]
    return out, payload, shows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libcimbar_hip.so built from the parent commit (set a)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    off, on = context(), context(salvage=True)
    geo = off.geo
    mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)

    class Out:
        def __init__(self):
            self.chunks, self.masks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)
            self.runs, self.roles, self.n_runs = mk(N, torch.int32), mk(N, torch.int32), mk(1, torch.int32)
            self.rchunks, self.rmasks = mk((N, geo.FRAME_BYTES), torch.uint8), mk(N, torch.int32)

    def once(dec, fr, o):
        return lambda: dec.decode_batch_once_device(fr.data_ptr(), N, o.chunks.data_ptr(), o.masks.data_ptr(), o.runs.data_ptr(), o.roles.data_ptr(),
                                                    o.rchunks.data_ptr(), o.rmasks.data_ptr(), o.n_runs.data_ptr(), min_agree_permille=MIN_AGREE, stream=stream)

    def combined(dec, fr, o):
        return lambda: dec.decode_batch_combined_device(fr.data_ptr(), N, o.chunks.data_ptr(), o.masks.data_ptr(), o.runs.data_ptr(), o.rchunks.data_ptr(),
                                                        o.rmasks.data_ptr(), o.n_runs.data_ptr(), stream=stream)

    def delivered(o, payload, shows):
        """the complete rows of a call, the distinct displayed frames among them, and whether every delivered chunk is the payload's"""
        nr = int(o.n_runs.item())
        rm = o.rmasks.cpu().numpy().view(np.uint32)[:nr]
        rc = o.rchunks.cpu().numpy()[:nr].reshape(nr, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        runs = o.runs.cpu().numpy()
        frame = np.full(nr, -1, np.int64)
        for k in range(N):                                                   # a row's frame: that of its members that show one whole
            if runs[k] >= 0 and shows[k] >= 0:
                frame[runs[k]] = shows[k]
        full = rm == geo.FULL_MASK
        ok = True
        for r in range(nr):
            if frame[r] < 0:
                continue
            want = payload[frame[r]].reshape(geo.CHUNKS_PER_FRAME, geo.CHUNK)
            ok = ok and all((rc[r, j] == want[j]).all() for j in range(geo.CHUNKS_PER_FRAME) if (int(rm[r]) >> j) & 1)
        return {"rows": nr, "complete_rows": int(full.sum()), "complete_frames": int(len(set(frame[full & (frame >= 0)].tolist()))),
                "every_delivered_chunk_is_the_payload": bool(ok)}

    roles_of = lambda o: dict(zip(("unusable", "skipped", "representative", "fallback", "torn"), np.bincount(o.roles.cpu().numpy() + 1, minlength=5).tolist()))
    res = {"mode": MODE, "captures": N, "reps": a.reps, "min_agree_permille": MIN_AGREE, "line_permille": LINE}

    # (a) clean runs of three, a torn capture after each
    fr, payload, shows = captures(off, dev, wiped=False)
    outs = {k: Out() for k in ("off", "on", "parent_1", "parent_2")}
    calls = {"off": once(off, fr, outs["off"]), "on": once(on, fr, outs["on"])}
    parents = []
    if a.parent_lib:
        parents = [context(a.parent_lib), context(a.parent_lib)]
        calls["parent_1"], calls["parent_2"] = once(parents[0], fr, outs["parent_1"]), once(parents[1], fr, outs["parent_2"])
    t = timed(calls, a.reps, dev)
    sa = summary(t)
    med = {k: v["median_ms"] for k, v in sa.items()}
    ca = {"times": sa, "on_minus_off_us": round((med["on"] - med["off"]) * 1000, 1), "roles": roles_of(outs["on"]),
          "off": delivered(outs["off"], payload, shows), "on": delivered(outs["on"], payload, shows),
          "same_outputs": bool(all(torch.equal(getattr(outs["off"], k), getattr(outs["on"], k)) for k in ("chunks", "masks", "runs", "roles", "rchunks", "rmasks"))),
          "salvaged_runs": int((on.tap_once_salvage(N)[:, [0, 4]] >= 0).any(axis=1).sum())}
    if parents:
        both = t["parent_1"] + t["parent_2"]
        ca["parent_spread_ms"] = [round(min(both), 4), round(max(both), 4)]
        ca["parent_medians_ms"] = sorted([med["parent_1"], med["parent_2"]])
        ca["on_inside_the_parents_spread"] = bool(min(both) <= med["on"] <= max(both))
        ca["off_inside_the_parents_spread"] = bool(min(both) <= med["off"] <= max(both))
        ca["same_outputs_as_the_parent"] = bool(all(torch.equal(getattr(outs["parent_1"], k), getattr(outs["on"], k)) for k in ("chunks", "masks", "runs", "roles", "rchunks", "rmasks")))
    res["clean_runs_of_three_torn_after_each"] = ca
    for p in parents:
        p.close()
    del fr

    # (b) a wiped run of one, the torn capture beside it, a clean run of two
    fr, payload, shows = captures(off, dev, wiped=True)
    o_off, o_on, o_cb = Out(), Out(), Out()
    cb_dec = D.HipDecoder(0, MODE)
    t = timed({"once_off": once(off, fr, o_off), "once_on": once(on, fr, o_on), "combined": combined(cb_dec, fr, o_cb)}, a.reps, dev)
    sb = summary(t)
    cb = {"times": sb, "once_off": delivered(o_off, payload, shows), "once_on": delivered(o_on, payload, shows), "combined": delivered(o_cb, payload, shows),
          "roles": roles_of(o_on), "salvaged_runs": int((on.tap_once_salvage(N)[:, [0, 4]] >= 0).any(axis=1).sum()),
          "on_minus_off_ms": round(sb["once_on"]["median_ms"] - sb["once_off"]["median_ms"], 4),
          "on_minus_combined_ms": round(sb["once_on"]["median_ms"] - sb["combined"]["median_ms"], 4)}
    cb["on_delivers_strictly_more_complete_frames"] = bool(cb["once_on"]["complete_frames"] > cb["once_off"]["complete_frames"])
    res["wiped_run_of_one_torn_clean_pair"] = cb
    for d in (off, on, cb_dec):
        d.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
