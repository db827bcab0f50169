"""Device time of torn-capture stitching against the plain batch decode, mode 68, on captures already in device memory, and what it delivers.

1 024 captures, two sets:
  clean   distinct frames rendered by the device encoder: no pair shares a band, so the stitched call adds S1, S2 and Reed-Solomon launches
          that return at once
  torn    every capture torn along a pixel row: capture k shows frame k above its tear and frame k + 1 below it. The tear moves down by
          --drift pixel rows from capture to capture and wraps; consecutive captures share the rows between their tears (none where it wraps)
Per set, decode_batch and decode_batch_stitched (device outputs) alternate within one run, `--reps` times each after a warm-up; the median
and the spread of the per-call times are reported, with the chunks the captures deliver alone and the chunks the stitched slots add.
Prints one JSON line; --out writes it to a file as well.

    python tools/stitch_bench.py [--n 1024] [--reps 20] [--drift 297] [--out profiles/r13_stitch_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--drift", type=int, default=297)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    dec = D.HipDecoder(0, mode)
    geo = dec.geo
    payload = framegen.synth_payload(n + 1, seed=13, mode=mode).numpy().reshape(n + 1, -1)
    frames = dec.encode_batch(payload)
    sets = {"clean": torch.from_numpy(frames[:n]).to(dev)}
    torn = frames[:n].copy()
    lo, span = 40, geo.IMG_H - 80                                      # the tears stay off the frame's first and last rows
    tears = [lo + (k * a.drift) % span for k in range(n)]
    for k in range(n):
        torn[k, tears[k]:] = frames[k + 1, tears[k]:]
    sets["torn"] = torch.from_numpy(torn).to(dev)
    shared = sum(1 for k in range(n - 1) if tears[k + 1] > tears[k])   # pairs whose captures share a band of frame k + 1
    del torn
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    schunks = torch.empty((2 * (n - 1), geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    smasks = torch.empty(2 * (n - 1), dtype=torch.int32, device=dev)
    d_tears = torch.empty((n - 1, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": mode, "captures": n, "reps": a.reps, "drift_rows": a.drift, "pairs_sharing_a_band": shared, "sets": {}}
    for name, fr in sets.items():
        calls = {
            "decode_batch": lambda: dec.decode_batch_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), stream=stream),
            "decode_batch_stitched": lambda: dec.decode_batch_stitched_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(),
                                                                             smasks.data_ptr(), d_tears.data_ptr(), axis=0, stream=stream),
        }
        for f in calls.values():
            f()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                torch.cuda.synchronize(dev)
                times[k].append(t0.elapsed_time(t1))
        pm = masks.cpu().numpy().view(np.uint32)
        sm = smasks.cpu().numpy().view(np.uint32)
        tr = d_tears.cpu().numpy()
        sc = schunks.cpu().numpy().reshape(2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK)
        # a stitched chunk is genuine when it is the payload chunk of one of the three frames the pair's captures show
        p = payload.reshape(n + 1, geo.CHUNKS_PER_FRAME, geo.CHUNK)
        wrong = 0
        for slot in np.flatnonzero(sm):
            k = slot // 2
            for j in range(geo.CHUNKS_PER_FRAME):
                if (int(sm[slot]) >> j) & 1 and not any((sc[slot, j] == p[q, j]).all() for q in range(k, min(k + 3, n + 1))):
                    wrong += 1
        base, st = statistics.median(times["decode_batch"]), statistics.median(times["decode_batch_stitched"])
        pop = lambda m: int(sum(bin(int(x)).count("1") for x in m))
        res["sets"][name] = {"decode_batch_ms": round(base, 4), "decode_batch_ms_min_max": [round(min(times["decode_batch"]), 4), round(max(times["decode_batch"]), 4)],
                             "decode_batch_stitched_ms": round(st, 4),
                             "decode_batch_stitched_ms_min_max": [round(min(times["decode_batch_stitched"]), 4), round(max(times["decode_batch_stitched"]), 4)],
                             "overhead_pct": round(100.0 * (st - base) / base, 2), "candidate_pairs": int((tr[:, 0] >= 0).sum()),
                             "capture_chunks": pop(pm), "captures_full": int((pm == geo.FULL_MASK).sum()),
                             "stitched_chunks_direction0": pop(sm[0::2]), "stitched_full_direction0": int((sm[0::2] == geo.FULL_MASK).sum()),
                             "stitched_chunks_direction1": pop(sm[1::2]), "stitched_chunks_not_genuine": wrong}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
