"""Device time of the stitched decode's erasure retry (cimbar_hip_set_stitch_erasure) and what it delivers, mode 68, on captures already in
device memory, device outputs. The torn set is tools/stitch_bench.py's: 1 024 captures, capture k showing frame k above its tear and frame
k + 1 below it, the tear moving down by --drift rows per capture.

  (a) undamaged   the setting off against on. Every stitched slot is complete or not live, so every workgroup of the two retry kernels
                  should return at its first test: `on` is expected inside the spread of two `off` contexts timed in the same alternation.
  (b) noisy       the same set with --noise of every capture's cells overwritten with random pixels, so that the off run loses chunks:
                  chunks and full frames the stitched slots deliver, off against on, and the time of each.
Three contexts (off, on, off) with both erasure settings on alternate within one run, --reps times each after a warm-up; medians with min-max.
Every chunk reported is checked against the payload of the three frames its pair shows. Prints one JSON line; --out writes it as well.

    python tools/stitch_erasure_bench.py [--n 1024] [--reps 20] [--drift 297] [--noise 0.03] [--out profiles/stitch_erasure_bench.json]
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
    ap.add_argument("--noise", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    decs = {"off_a": D.HipDecoder(0, mode), "on": D.HipDecoder(0, mode), "off_b": D.HipDecoder(0, mode)}
    for name, d in decs.items():
        d.set_erasure_decode(6)
        d.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED)
        d.set_stitch_erasure(name == "on")
    geo = decs["on"].geo
    payload = framegen.synth_payload(n + 1, seed=13, mode=mode).numpy().reshape(n + 1, -1)
    frames = decs["on"].encode_batch(payload)
    torn = frames[:n].copy()
    lo, span = 40, geo.IMG_H - 80
    tears = [lo + (k * a.drift) % span for k in range(n)]
    for k in range(n):
        torn[k, tears[k]:] = frames[k + 1, tears[k]:]
    del frames
    sets = {"undamaged": torch.from_numpy(torn).to(dev)}
    g = np.random.default_rng(17)
    xy = geo.cell_positions()
    per = int(round(a.noise * geo.NCELLS))
    for k in range(n):
        for c in g.choice(geo.NCELLS, per, replace=False):
            x, y = xy[c]
            torn[k, y:y + 8, x:x + 8] = g.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    sets["noisy"] = torch.from_numpy(torn).to(dev)
    del torn
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    schunks = torch.empty((2 * (n - 1), geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    smasks = torch.empty(2 * (n - 1), dtype=torch.int32, device=dev)
    d_tears = torch.empty((n - 1, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = payload.reshape(n + 1, geo.CHUNKS_PER_FRAME, geo.CHUNK)
    pop = lambda m: int(sum(bin(int(x)).count("1") for x in m))
    res = {"mode": mode, "captures": n, "reps": a.reps, "drift_rows": a.drift, "noise_cells_per_capture": per, "sets": {}}
    for name, fr in sets.items():
        call = lambda d: d.decode_batch_stitched_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(),
                                                        d_tears.data_ptr(), axis=0, stream=stream)
        for d in decs.values():
            d.reset_ccm()
            call(d)
        torch.cuda.synchronize(dev)
        times = {k: [] for k in decs}
        for _ in range(a.reps):
            for k, d in decs.items():
                d.reset_ccm()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(d)
                t1.record()
                torch.cuda.synchronize(dev)
                times[k].append(t0.elapsed_time(t1))
        out = {}
        for k in ("off_a", "on"):                                    # what each delivers: one more call, read back
            decs[k].reset_ccm()
            call(decs[k])
            torch.cuda.synchronize(dev)
            sm = smasks.cpu().numpy().view(np.uint32)
            sc = schunks.cpu().numpy().reshape(2 * (n - 1), geo.CHUNKS_PER_FRAME, geo.CHUNK)
            wrong = 0
            for slot in np.flatnonzero(sm):
                q0 = slot // 2
                for j in range(geo.CHUNKS_PER_FRAME):
                    if (int(sm[slot]) >> j) & 1 and not any((sc[slot, j] == p[q, j]).all() for q in range(q0, min(q0 + 3, n + 1))):
                        wrong += 1
            key = "off" if k == "off_a" else "on"
            out[key + "_stitched_chunks"] = pop(sm)
            out[key + "_stitched_full_frames"] = int((sm == geo.FULL_MASK).sum())
            out[key + "_stitched_chunks_not_genuine"] = wrong
            out[key + "_candidate_pairs"] = int((d_tears.cpu().numpy()[:, 0] >= 0).sum())
        for k, t in times.items():
            out[k + "_ms"] = round(statistics.median(t), 4)
            out[k + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        res["sets"][name] = out
    for d in decs.values():
        d.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
