"""The relaxed flood against the default policy, same library, same box, alternated in one run (one JSON line):

    python tools/relaxed_flood_bench.py [--n 256] [--reps 5] [--rounds 3] [--threshold 12] [--out FILE, default profiles/relaxed_flood_bench.json]

  captures  the 1080p RGB8 capture set of tools/capture_formats_bench.py through cimbar_hip_scan_extract_decode_batch_fmt
  frames    noisy / rescaled / shifted frames through cimbar_hip_decode_batch

Per set and policy (`off` = the default: exact replay; `on` = cimbar_hip_set_relaxed_flood(threshold, fallback 1)):
  call_ms          the whole call, median over `rounds` rounds of `reps` back-to-back calls timed with one event pair, policies interleaved
  flood_ms, rs_symbols_ms   the stage times of one call with cimbar_hip_enable_timing (the relaxed launches fall into these two slots)
  chunks           chunks delivered (bits set in the masks) by one call
  and for `on`: frames flooded in rounds, the share accepted, frames handed to the exact replay, rounds per frame."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libcimbar_amd import decoder as D, framegen            # noqa: E402
from tests import frames as F                               # noqa: E402
from tests.test_oracle_vs_ref import CAMERA_CASES           # noqa: E402


def distorted_frames(clean, n):
    kinds = [lambda c, k: F.add_noise(c, 40 + 20 * (k % 5), k), lambda c, k: F.rescale(c, 3 + k % 5), lambda c, k: F.add_noise(F.shift(c, 1 + k % 2, -2), 60, k),
             lambda c, k: F.add_noise(F.rescale(c, 5), 60, k), lambda c, k: F.shift(c, -3 + k % 7, 3 - k % 5)]
    base = [kinds[k % len(kinds)](clean[k % len(clean)], k) for k in range(min(n, 40))]
    return np.ascontiguousarray(np.stack([base[k % len(base)] for k in range(n)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=D.RELAXED_FLOOD_SUGGESTED)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "relaxed_flood_bench.json"))
    a = ap.parse_args()
    w, h, n = 1920, 1080, a.n
    synth = framegen.FrameSynth("cpu")
    _, frames = F.clean_frames(synth, len(CAMERA_CASES), seed=90)
    rgbs = [F.camera_frame(frames[k], width=w, height=h, quad=q, background=bg, blur=bl) for k, (bg, q, bl) in enumerate(CAMERA_CASES)]
    d_caps = torch.from_numpy(np.stack([rgbs[k % len(rgbs)] for k in range(n)])).cuda()
    _, clean = F.clean_frames(synth, 8, seed=123)
    d_frames = torch.from_numpy(distorted_frames(clean, n)).cuda()
    dec = {"off": D.HipDecoder(0), "on": D.HipDecoder(0)}
    dec["on"].set_relaxed_flood(a.threshold, fallback=True)
    lib = dec["off"]._lib
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    d_chunks = torch.empty((n, 12, 625), dtype=torch.uint8, device="cuda")
    d_masks = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(policy, which):
        d = dec[policy]
        if which == "captures":
            rc = lib.cimbar_hip_scan_extract_decode_batch_fmt(d._ctx, P(d_caps), w, h, 3, n, D.MEM_DEVICE, 1, 2, P(d_chunks), P(d_masks), P(d_status), D.MEM_DEVICE, st)
        else:
            rc = lib.cimbar_hip_decode_batch(d._ctx, P(d_frames), n, D.MEM_DEVICE, 0, 2, P(d_chunks), P(d_masks), D.MEM_DEVICE, st)
        if rc < 0:
            raise RuntimeError(f"{which} / {policy}: {rc} {lib.cimbar_hip_last_error(d._ctx)}")

    res = {"n": n, "threshold": a.threshold, "fallback": 1, "reps": a.reps, "rounds": a.rounds, "sets": {}}
    for which in ("captures", "frames"):
        times = {"off": [], "on": []}
        for policy in times:                                  # warm-up: allocations
            call(policy, which)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for policy in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call(policy, which)
                e1.record()
                torch.cuda.synchronize()
                times[policy].append(e0.elapsed_time(e1) / a.reps)
        row = {}
        for policy in times:
            d = dec[policy]
            med = statistics.median(times[policy])
            r = {"call_ms": round(med, 3), "call_spread": round((max(times[policy]) - min(times[policy])) / med, 3)}
            d.reset_ccm()
            if policy == "on":
                d.set_relaxed_flood(a.threshold, fallback=True)    # clears the counts: they then describe the one call below
            d.enable_timing(True)
            call(policy, which)
            torch.cuda.synchronize()
            stages = d.stage_times()
            d.enable_timing(False)
            r["flood_ms"] = round(stages["flood"], 3)
            r["rs_symbols_ms"] = round(stages["rs_symbols"], 3)
            masks = d_masks.cpu().numpy().astype(np.uint32)
            r["chunks"] = int(sum(bin(int(m)).count("1") for m in masks))
            path = d.tap(D.TAP_FLOOD_PATH, n)
            r["paths"] = {str(p): int((path == p).sum()) for p in range(4)}
            if policy == "on":
                flooded, accepted, handed, rounds = d.relaxed_flood_stats()
                r.update({"flooded_in_rounds": flooded, "accepted": accepted, "handed_to_exact": handed,
                          "accepted_share": round(accepted / flooded, 3) if flooded else None,
                          "rounds_per_frame": round(rounds / flooded, 1) if flooded else None})
            row[policy] = r
        res["sets"][which] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
