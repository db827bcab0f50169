"""Time per call of repeat-capture skipping across calls (decode_batch_once_stream) against the plain one-capture decode_batch, mode 68, on
captures already in device memory, handed over ONE PER CALL, and what both deliver.

96 calls: 32 displayed frames in runs of three, two sets, seeded (those of tools/repeat_skip_bench.py):
  drifted  every run made from one clean frame X as (rescale(X, +6), that plus noise 40, that shifted by (1, 0)): every capture leaves the
           parallel pass and takes the flood
  clean    every run three copies of X: no capture takes the flood
Per set, a pass of 96 decode_batch calls (n = 1) and a pass of 96 stream calls (device outputs) alternate within one process, `--reps` times
each after a warm-up. A pass is timed on the host clock from its first call to a device synchronisation behind its last, so the stream call's
read-backs and every launch gap count; both passes start from a reset colour matrix, the stream pass from a reset carry. Reported: the median
and the range of the per-call time (pass time / 96), the decoded and skipped calls, the chunks per displayed frame both deliver (the plain
calls': the OR over the frame's three captures; the stream calls': rmasks of the run's last call) and whether every reported chunk is genuine.
Prints one JSON line; --out writes it to a file as well.

    python tools/repeat_stream_bench.py [--calls 96] [--reps 20] [--out profiles/repeat_stream_bench.json]
    python tools/repeat_stream_bench.py --stream-only --sets clean      (one pass of stream calls and nothing else, for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libcimbar_amd import decoder as D  # noqa: E402
from libcimbar_amd import framegen  # noqa: E402
from tests import frames as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=96)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", default="drifted,clean")
    ap.add_argument("--stream-only", action="store_true", help="one pass of stream calls per set and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.calls
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
    mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    # every call writes slots of its own, so that a pass leaves all its results behind
    chunks, masks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    ochunks, omasks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    runs, roles, n_runs, cont = mk(n, torch.int32), mk(n, torch.int32), mk(n, torch.int32), mk(n, torch.int32)
    rchunks, rmasks = mk((n, geo.FRAME_BYTES), torch.uint8), mk(n, torch.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fb = geo.FRAME_RGB_BYTES
    pop = lambda m: [bin(int(x)).count("1") for x in m]
    res = {"mode": mode, "calls": n, "displayed_frames": shown, "reps": a.reps, "sets": {}}
    for name, fr in sets.items():
        def plain_pass():
            dec.reset_ccm()
            for k in range(n):
                dec.decode_batch_device(fr.data_ptr() + k * fb, 1, chunks.data_ptr() + k * geo.FRAME_BYTES, masks.data_ptr() + 4 * k, stream=stream)

        def stream_pass():
            dec.reset_ccm()
            dec.once_stream_reset()
            for k in range(n):
                dec.decode_batch_once_stream_device(fr.data_ptr() + k * fb, 1, ochunks.data_ptr() + k * geo.FRAME_BYTES, omasks.data_ptr() + 4 * k,
                                                    runs.data_ptr() + 4 * k, roles.data_ptr() + 4 * k, rchunks.data_ptr() + k * geo.FRAME_BYTES,
                                                    rmasks.data_ptr() + 4 * k, n_runs.data_ptr() + 4 * k, cont.data_ptr() + 4 * k, stream=stream)

        passes = {"decode_batch": plain_pass, "decode_batch_once_stream": stream_pass}
        if a.stream_only:
            stream_pass()
            torch.cuda.synchronize(dev)
            continue
        for f in passes.values():
            f()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in passes}
        for _ in range(a.reps):
            for k, f in passes.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(dev)
                times[k].append((time.perf_counter() - t0) * 1e3 / n)
        pm = masks.cpu().numpy().view(np.uint32)
        rm = rmasks.cpu().numpy().view(np.uint32)
        ro, co = roles.cpu().numpy(), cont.cpu().numpy()
        plain_or = np.zeros(shown, np.uint32)
        np.bitwise_or.at(plain_or, truth, pm)
        # a call continues the run of the call before exactly where both show one displayed frame
        same_runs = bool((co == (np.arange(n) % 3 != 0)).all())
        last = np.minimum(3 * np.arange(shown) + 2, n - 1)                 # the last call of every displayed frame: its row is cumulative
        run_masks = rm[last]
        rc = rchunks.cpu().numpy()
        wrong = sum(1 for r in range(shown) for j in range(geo.CHUNKS_PER_FRAME)
                    if (int(run_masks[r]) >> j) & 1 and not (rc[last[r], j * geo.CHUNK:(j + 1) * geo.CHUNK] == payload[r, j * geo.CHUNK:(j + 1) * geo.CHUNK]).all()) if same_runs else -1
        base, strm = statistics.median(times["decode_batch"]), statistics.median(times["decode_batch_once_stream"])
        hist = lambda v: {str(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))}
        rnd = lambda v: round(v, 4)
        res["sets"][name] = {
            "decode_batch_ms_per_call": rnd(base), "decode_batch_ms_per_call_min_max": [rnd(min(times["decode_batch"])), rnd(max(times["decode_batch"]))],
            "once_stream_ms_per_call": rnd(strm), "once_stream_ms_per_call_min_max": [rnd(min(times["decode_batch_once_stream"])), rnd(max(times["decode_batch_once_stream"]))],
            "stream_over_plain": rnd(strm / base), "roles": hist(ro), "decoded_calls": int((ro > 0).sum()), "skipped_calls": int((ro == 0).sum()),
            "runs_are_the_displayed_frames": same_runs,
            "plain_chunks_per_frame": hist(pop(plain_or)), "stream_chunks_per_frame": hist(pop(run_masks)),
            "plain_complete_frames": int((plain_or == geo.FULL_MASK).sum()), "stream_complete_frames": int((run_masks == geo.FULL_MASK).sum()),
            "stream_chunks_not_genuine": int(wrong)}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
