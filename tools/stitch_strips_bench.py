"""Device time of torn-capture stitching strip by strip (cimbar_hip_set_stitch_strips 8) against whole lines (strips 1), mode 68, on
captures already in device memory, and what each recovers from slanted tears.

1 024 captures, the clean set and the torn set of tools/stitch_bench.py and two slanted sets:
  clean    distinct frames: no pair shares a band
  torn     capture k shows frame k above a straight tear and frame k + 1 below it; the tear moves down by --drift pixel rows per capture
  slanted  the torn set cut with a tear that rises --rise grid lines across the frame (tests/stitch_strips_cases.cut_slanted, sharp)
  slanted_close  the same slant with the tear moving --close-drift pixel rows per capture: the two tears of a pair lie fewer lines apart
           than 3/4 of the rise, the regime the strips are for
Per set, decode_batch_stitched (device outputs) with strips 1 and with strips 8 alternate within one process, `--reps` times each after a
warm-up; the medians, their difference and the interquartile spread of the strips-1 times are reported, with the candidate pairs, the
stitched chunks and the full slots of either setting and a count of stitched chunks that are no chunk of the frames the pair shows.
Prints one JSON line; --out writes it to a file as well.

    python tools/stitch_strips_bench.py [--n 1024] [--reps 20] [--out profiles/stitch_strips_bench.json]
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


def torn_set(frames, n, tears, rise_px):
    """capture k: frame k in front of the tear tears[k] + rise_px * u / (w - 1) at pixel column u, frame k + 1 from it on"""
    h, w = frames.shape[1:3]
    rows = np.arange(h, dtype=np.float64)[:, None]
    ramp = rise_px * np.arange(w, dtype=np.float64)[None, :] / (w - 1)
    out = np.empty_like(frames[:n])
    for k in range(n):
        out[k] = np.where((rows >= tears[k] + ramp)[..., None], frames[k + 1], frames[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--drift", type=int, default=297)
    ap.add_argument("--close-drift", type=int, default=54)
    ap.add_argument("--rise", type=int, default=10)
    ap.add_argument("--strips", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    dec = D.HipDecoder(0, mode)
    geo = dec.geo
    payload = framegen.synth_payload(n + 1, seed=13, mode=mode).numpy().reshape(n + 1, -1)
    frames = dec.encode_batch(payload)
    rise_px = a.rise * geo.PITCH
    lo, span = 40, geo.IMG_H - 80 - rise_px                            # the tears stay off the frame's first and last rows
    tears = {d: [lo + (k * d) % span for k in range(n)] for d in (a.drift, a.close_drift)}
    plans = {"clean": None, "torn": (a.drift, 0), "slanted": (a.drift, rise_px), "slanted_close": (a.close_drift, rise_px)}
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    schunks = torch.empty((2 * (n - 1), geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    smasks = torch.empty(2 * (n - 1), dtype=torch.int32, device=dev)
    d_tears = torch.empty((n - 1, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = payload.reshape(n + 1, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    pop = lambda m: int(sum(bin(int(x)).count("1") for x in m))
    res = {"mode": mode, "captures": n, "reps": a.reps, "rise_lines": a.rise, "strips": a.strips, "sets": {}}
    for name, plan in plans.items():
        fr = torch.from_numpy(frames[:n] if plan is None else torn_set(frames, n, tears[plan[0]], plan[1])).to(dev)
        settings = (1, a.strips)

        def call(S):
            dec.set_stitch_strips(S)
            dec.decode_batch_stitched_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(),
                                             d_tears.data_ptr(), axis=0, stream=stream)

        for S in settings:
            call(S)
        torch.cuda.synchronize(dev)
        times = {S: [] for S in settings}
        for _ in range(a.reps):
            for S in settings:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(S)
                t1.record()
                torch.cuda.synchronize(dev)
                times[S].append(t0.elapsed_time(t1))
        row = {}
        if plan is not None:
            row["drift_rows"] = plan[0]
            row["pairs_sharing_a_band"] = sum(1 for k in range(n - 1) if tears[plan[0]][k + 1] > tears[plan[0]][k])
        for S in settings:
            call(S)
            torch.cuda.synchronize(dev)
            sm, tr = smasks.cpu().numpy().view(np.uint32), d_tears.cpu().numpy()
            sc = schunks.cpu().numpy().reshape(2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK)
            # a stitched chunk is genuine when it is the payload chunk of one of the three frames the pair's captures show
            wrong = 0
            for slot in np.flatnonzero(sm):
                k = slot // 2
                for j in range(geo.CHUNKS_PER_FRAME):
                    if (int(sm[slot]) >> j) & 1 and not any((sc[slot, j] == p[q, j]).all() for q in range(k, min(k + 3, n + 1))):
                        wrong += 1
            q = statistics.quantiles(times[S], n=4)
            row["strips_%d" % S] = {"ms": round(statistics.median(times[S]), 4), "ms_quartiles": [round(q[0], 4), round(q[2], 4)],
                                    "ms_min_max": [round(min(times[S]), 4), round(max(times[S]), 4)],
                                    "candidate_pairs": int((tr[:, 0] >= 0).sum()), "stitched_chunks_direction0": pop(sm[0::2]),
                                    "stitched_full_direction0": int((sm[0::2] == geo.FULL_MASK).sum()),
                                    "stitched_chunks_direction1": pop(sm[1::2]), "stitched_chunks_not_genuine": wrong}
        base, st = row["strips_1"], row["strips_%d" % a.strips]
        row["difference_ms"] = round(st["ms"] - base["ms"], 4)
        row["strips_1_interquartile_ms"] = round(base["ms_quartiles"][1] - base["ms_quartiles"][0], 4)
        row["difference_pct"] = round(100.0 * (st["ms"] - base["ms"]) / base["ms"], 2)
        res["sets"][name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
        del fr
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
