"""Device time of repeat-capture skipping (decode_batch_once) against the plain batch decode, mode 68, on captures already in device memory,
and what both deliver.

1 024 captures in runs of three (341 displayed frames and one capture of a 342nd), two sets, seeded:
  drifted  every run made from one clean frame X as (rescale(X, +6), that plus noise 40, that shifted by (1, 0)): every capture leaves the
           parallel pass and takes the flood
  clean    every run three copies of X: no capture takes the flood, so the signature pass is expected to cost about what it saves
Per set, decode_batch and decode_batch_once (device outputs) alternate within one process, `--reps` times each after a warm-up, timed with
device events around the call (the once-call's two read-backs included); the median and the spread of the per-call times are reported, with the
roles histogram, the chunks per displayed frame both calls deliver (the plain call's: the OR over the frame's three captures) and whether the
two deliver the same set of complete frames.
Prints one JSON line; --out writes it to a file as well.

    python tools/repeat_skip_bench.py [--n 1024] [--tile 1] [--reps 20] [--out profiles/repeat_skip_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", default="drifted,clean")
    ap.add_argument("--tile", type=int, default=1, help="repeat each set that many times on the device: --n 1024 --tile 3 times 3 072 captures")
    ap.add_argument("--once-only", action="store_true", help="one decode_batch_once call per set and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    shown = (n + 2) // 3
    dec = D.HipDecoder(0, mode)
    geo = dec.geo
    payload = framegen.synth_payload(shown, seed=29, mode=mode).numpy().reshape(shown, -1)
    frames = dec.encode_batch(payload)
    truth = np.arange(n) // 3
    sets = {}
    if "drifted" in a.sets:
        buf = np.empty((n, *geo.FRAME_SHAPE), np.uint8)
        for r in range(shown):
            v0 = F.rescale(frames[r], 6)
            v1 = F.add_noise(v0, 40, 1000 + r)
            for j, v in enumerate((v0, v1, F.shift(v1, 1, 0))):
                if 3 * r + j < n:
                    buf[3 * r + j] = v
        sets["drifted"] = torch.from_numpy(buf).to(dev)
        del buf
    if "clean" in a.sets:
        sets["clean"] = torch.from_numpy(frames[truth]).to(dev)
    if a.tile > 1:
        # (a set's last run is followed by its first: another displayed frame, so the runs stay what they are)
        sets = {k: v.repeat(a.tile, 1, 1, 1) for k, v in sets.items()}
        truth = np.concatenate([t * shown + truth for t in range(a.tile)])
        payload = np.tile(payload, (a.tile, 1))
        n, shown = n * a.tile, shown * a.tile
    mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    chunks, masks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    ochunks, omasks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    runs, roles, n_runs = mk(n, torch.int32), mk(n, torch.int32), mk(1, torch.int32)
    rchunks, rmasks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pop = lambda m: [bin(int(x)).count("1") for x in m]
    res = {"mode": mode, "captures": n, "displayed_frames": shown, "reps": a.reps, "sets": {}}
    for name, fr in sets.items():
        calls = {
            "decode_batch": lambda: dec.decode_batch_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), stream=stream),
            "decode_batch_once": lambda: dec.decode_batch_once_device(fr.data_ptr(), n, ochunks.data_ptr(), omasks.data_ptr(), runs.data_ptr(), roles.data_ptr(),
                                                                      rchunks.data_ptr(), rmasks.data_ptr(), n_runs.data_ptr(), stream=stream),
        }
        if a.once_only:
            calls["decode_batch_once"]()
            torch.cuda.synchronize(dev)
            continue
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
        rm = rmasks.cpu().numpy().view(np.uint32)
        ro = roles.cpu().numpy()
        ru = runs.cpu().numpy()
        nr = int(n_runs.item())
        plain_or = np.zeros(shown, np.uint32)
        np.bitwise_or.at(plain_or, truth, pm)
        # a run of the once-call is one displayed frame when its captures are exactly that frame's
        same_runs = nr == shown and (ru == truth).all()
        plain_full = set(np.flatnonzero(plain_or == geo.FULL_MASK).tolist())
        once_full = set(np.flatnonzero(rm[:nr] == geo.FULL_MASK).tolist())
        # ... and every chunk it reports is that frame's payload
        rc = rchunks.cpu().numpy()
        wrong = sum(1 for r in range(min(nr, shown)) for j in range(geo.CHUNKS_PER_FRAME)
                    if (int(rm[r]) >> j) & 1 and not (rc[r, j * geo.CHUNK:(j + 1) * geo.CHUNK] == payload[r, j * geo.CHUNK:(j + 1) * geo.CHUNK]).all()) if same_runs else -1
        base, once = statistics.median(times["decode_batch"]), statistics.median(times["decode_batch_once"])
        hist = lambda v: {str(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))}
        res["sets"][name] = {
            "decode_batch_ms": round(base, 4), "decode_batch_ms_min_max": [round(min(times["decode_batch"]), 4), round(max(times["decode_batch"]), 4)],
            "decode_batch_once_ms": round(once, 4), "decode_batch_once_ms_min_max": [round(min(times["decode_batch_once"]), 4), round(max(times["decode_batch_once"]), 4)],
            "once_over_plain": round(once / base, 4), "roles": hist(ro), "runs": nr, "runs_are_the_displayed_frames": bool(same_runs),
            "plain_chunks_per_frame": hist(pop(plain_or)), "once_chunks_per_run": hist(pop(rm[:nr])),
            "plain_complete_frames": len(plain_full), "once_complete_runs": len(once_full), "same_complete_set": bool(same_runs and plain_full == once_full),
            "once_chunks_not_genuine": int(wrong)}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
