"""Device time of multi-capture decoding against the plain batch decode, mode 68, on captures already in device memory.

1 024 captures in groups of three (341 frames rendered by the device encoder, each captured three times, the last frame once), two sets:
  clean     the three captures identical: nearly every cell unanimous, one Reed-Solomon pass per group
  damaged   each capture with a white, black or noise disc at a place the other two leave clean (radius 0.19 of the frame): the disputed
            cells take the full vote
Per set, decode_batch and decode_batch_combined (device outputs) alternate within one run, `--reps` times each after a warm-up; the
median of the per-call times is reported. Prints one JSON line; --out writes it to a file as well.

    python tools/combine_bench.py [--n 1024] [--reps 20] [--out profiles/r09_combine_bench.json]
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

PLACES = [(0.50, 0.24), (0.26, 0.70), (0.74, 0.70)]
KINDS = ("white", "black", "noise")


def disc(frame, cx, cy, r, kind, g):
    h, w, _ = frame.shape
    yy, xx = np.ogrid[0:h, 0:w]
    d = (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * min(h, w)) ** 2
    if kind == "white":
        frame[d] = 255
    elif kind == "black":
        frame[d] = 0
    else:
        frame[d] = g.integers(0, 256, (int(d.sum()), 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    dec = D.HipDecoder(0, mode)
    geo = dec.geo
    nframes = (n + 2) // 3
    payload = framegen.synth_payload(nframes, seed=9, mode=mode).numpy().reshape(nframes, -1)
    frames = dec.encode_batch(payload)
    idx = np.arange(n) // 3
    g = np.random.default_rng(1)
    sets = {}
    sets["clean"] = torch.from_numpy(frames[idx]).to(dev)
    damaged = frames[idx].copy()
    for k in range(n):
        cx, cy = PLACES[k % 3]
        disc(damaged[k], cx, cy, 0.19, KINDS[(k // 3 + k) % 3], g)
    sets["damaged"] = torch.from_numpy(damaged).to(dev)
    del damaged
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    groups = torch.empty(n, dtype=torch.int32, device=dev)
    gchunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    gmasks = torch.empty(n, dtype=torch.int32, device=dev)
    ng = torch.empty(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": mode, "captures": n, "group": 3, "reps": a.reps, "sets": {}}
    for name, fr in sets.items():
        calls = {
            "decode_batch": lambda: dec.decode_batch_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), stream=stream),
            "decode_batch_combined": lambda: dec.decode_batch_combined_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), groups.data_ptr(),
                                                                             gchunks.data_ptr(), gmasks.data_ptr(), ng.data_ptr(), stream=stream),
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
        gm = gmasks.cpu().numpy().view(np.uint32)[:int(ng.item())]
        pm = masks.cpu().numpy().view(np.uint32)
        base, comb = statistics.median(times["decode_batch"]), statistics.median(times["decode_batch_combined"])
        res["sets"][name] = {"decode_batch_ms": round(base, 4), "decode_batch_combined_ms": round(comb, 4),
                             "overhead_pct": round(100.0 * (comb - base) / base, 2), "n_groups": int(ng.item()),
                             "capture_chunks": int(sum(bin(int(x)).count("1") for x in pm)),
                             "group_chunks": int(sum(bin(int(x)).count("1") for x in gm)), "group_full": int((gm == geo.FULL_MASK).sum())}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
