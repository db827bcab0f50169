"""Device time of torn-capture stitching across calls against the plain calls, mode 68, on captures already in device memory, and what one
capture per call recovers. The sets are those of tools/stitch_bench.py: 1 024 captures, clean (distinct frames) and torn (capture k shows
frame k above its tear and frame k + 1 below it, the tear moving down --drift pixel rows per capture and wrapping). Device outputs throughout.

  (a) one stream call over the whole set against decode_batch_stitched: the two alternate in one run and process, `--reps` times each after
      a warm-up; medians, and the difference beside the baseline's interquartile spread
  (b) one capture per call, --inflight calls enqueued before one synchronisation: decode_batch_stitched_stream against decode_batch, the
      same alternation; per-call time = the whole burst / --inflight
  (c) --recovery: the torn set as --n calls of one capture. Exits non-zero unless the (slot, chunk) pairs delivered over all calls are what
      ONE decode_batch_stitched call delivers for the set -- the same chunk count, the same full-mask pairs, every chunk equal -- and
      decode_batch_stitched with n = 1 adds nothing.
Prints one JSON line and writes it to --out (profiles/stitch_stream_bench.json).

    python tools/stitch_stream_bench.py [--n 1024] [--reps 20] [--inflight 256] [--drift 297] [--recovery] [--out profiles/stitch_stream_bench.json]
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


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": round(statistics.median(ts), 5), "iqr_ms": [round(q[0], 5), round(q[2], 5)], "min_max_ms": [round(min(ts), 5), round(max(ts), 5)]}


def alternate(calls, reps, dev):
    """every call once as a warm-up, then `reps` rounds of each in turn -> {name: [ms, ...]}"""
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


def compare(times, base, new, scale=1.0):
    b, s = [t * scale for t in times[base]], [t * scale for t in times[new]]
    sb, ss = summary(b), summary(s)
    return {base: sb, new: ss, "difference_ms": round(ss["median_ms"] - sb["median_ms"], 5),
            "baseline_iqr_width_ms": round(sb["iqr_ms"][1] - sb["iqr_ms"][0], 5),
            "difference_pct": round(100.0 * (ss["median_ms"] - sb["median_ms"]) / sb["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=256)
    ap.add_argument("--drift", type=int, default=297)
    ap.add_argument("--recovery", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stitch_stream_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    m = min(a.inflight, n)
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
    del torn, frames
    frame_bytes = geo.IMG_W * geo.IMG_H * 3
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    schunks = torch.empty((2 * n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    smasks = torch.empty(2 * n, dtype=torch.int32, device=dev)
    d_tears = torch.empty((n, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": mode, "captures": n, "reps": a.reps, "inflight": m, "drift_rows": a.drift, "sets": {}}

    def one_per_call(fr, count, stitched):
        """`count` calls of one capture, outputs side by side as one call of `count` captures lays them out"""
        for k in range(count):
            src, c, mk = fr.data_ptr() + k * frame_bytes, chunks.data_ptr() + k * geo.FRAME_BYTES, masks.data_ptr() + 4 * k
            if stitched:
                dec.decode_batch_stitched_stream_device(src, 1, c, mk, schunks.data_ptr() + 2 * k * geo.FRAME_BYTES, smasks.data_ptr() + 8 * k,
                                                        d_tears.data_ptr() + 16 * k, axis=0, stream=stream)
            else:
                dec.decode_batch_device(src, 1, c, mk, stream=stream)

    for name, fr in sets.items():
        whole = {
            "decode_batch_stitched": lambda: dec.decode_batch_stitched_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(),
                                                                             smasks.data_ptr(), d_tears.data_ptr(), axis=0, stream=stream),
            "decode_batch_stitched_stream": lambda: dec.decode_batch_stitched_stream_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(),
                                                                                           schunks.data_ptr(), smasks.data_ptr(), d_tears.data_ptr(),
                                                                                           axis=0, stream=stream),
        }
        single = {"decode_batch": lambda: one_per_call(fr, m, False), "decode_batch_stitched_stream": lambda: one_per_call(fr, m, True)}
        res["sets"][name] = {"a_whole_set_per_call": compare(alternate(whole, a.reps, dev), "decode_batch_stitched", "decode_batch_stitched_stream"),
                             "b_one_capture_per_call": compare(alternate(single, a.reps, dev), "decode_batch", "decode_batch_stitched_stream", 1.0 / m)}

    ok = True
    if a.recovery:
        fr = sets["torn"]
        pop = lambda x: int(sum(bin(int(v)).count("1") for v in x))
        dec.reset_ccm()
        dec.decode_batch_stitched_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), schunks.data_ptr(), smasks.data_ptr(), d_tears.data_ptr(),
                                         axis=0, stream=stream)
        torch.cuda.synchronize(dev)
        want_m, want_sm = masks.cpu().numpy().view(np.uint32).copy(), smasks[:2 * (n - 1)].cpu().numpy().view(np.uint32).copy()
        want_sc = schunks[:2 * (n - 1)].cpu().numpy().copy()
        schunks.fill_(0xA5)
        smasks.fill_(-1)
        dec.reset_ccm()
        dec.stitch_stream_reset()
        one_per_call(fr, n, True)
        torch.cuda.synchronize(dev)
        got_m, got_sm, got_sc = masks.cpu().numpy().view(np.uint32), smasks.cpu().numpy().view(np.uint32), schunks.cpu().numpy()
        # the plain pair k (slots 2k, 2k + 1) is row 0 of call k + 1 (slots 2 (k + 1), 2 (k + 1) + 1); call 0's row has no partner
        same_masks = bool((got_sm[2:] == want_sm).all() and not got_sm[:2].any())
        same_chunks = bool((got_sc[2:] == want_sc).all() and not got_sc[:2].any())
        # what the plain stitched call adds when it is fed the same way: no slot exists for n = 1
        plain_added = 0
        dec.reset_ccm()
        for k in range(n):
            rc = dec.decode_batch_stitched_device(fr.data_ptr() + k * frame_bytes, 1, chunks.data_ptr() + k * geo.FRAME_BYTES, masks.data_ptr() + 4 * k,
                                                  None, None, None, axis=0, stream=stream)
            plain_added += int(rc != 0)
        torch.cuda.synchronize(dev)
        plain_m = masks.cpu().numpy().view(np.uint32)
        rec = {"calls": n, "capture_chunks": pop(got_m), "captures_full": int((got_m == geo.FULL_MASK).sum()),
               "stitched_chunks_one_call": pop(want_sm), "stitched_chunks_one_capture_per_call": pop(got_sm),
               "stitched_full_one_call": int((want_sm == geo.FULL_MASK).sum()), "stitched_full_one_capture_per_call": int((got_sm == geo.FULL_MASK).sum()),
               "masks_equal": same_masks, "chunks_equal": same_chunks, "capture_masks_equal": bool((got_m == want_m).all() and (plain_m == want_m).all()),
               "plain_stitched_one_capture_per_call_adds": plain_added}
        ok = same_masks and same_chunks and rec["capture_masks_equal"] and plain_added == 0 and pop(want_sm) > 0
        rec["ok"] = bool(ok)
        res["recovery"] = rec
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
