"""Device time of multi-capture decoding across calls against the plain combined call, mode 68, on captures already in device memory.

The sets of tools/combine_bench.py: 1 024 captures in groups of three, clean (the three captures identical) and damaged (a disc of radius
0.19 per capture at a place the other two leave clean). Three measurements, the compared calls alternating within one run, `--reps`
times each after a warm-up, medians:
  (a) one call over all n captures, device outputs: decode_batch_combined against decode_batch_combined_stream with a flush (what the
      stream call adds: one G1 pair, the member indirection, k_group_carry). The spread of the baseline is reported beside the overhead.
  (b) one capture per call, device outputs, `--calls` calls in flight on one stream and one synchronise at the end: decode_batch_combined
      with n = 1 against the stream call, time per capture.
  (c) the damaged set fed as n calls of one capture (host outputs): the chunks the groups deliver, plain combined against stream.
Prints one JSON line; --out writes it to a file as well.

    python tools/combine_stream_bench.py [--n 1024] [--reps 20] [--calls 256] [--out profiles/r12_combine_stream_bench.json]
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
from tools.combine_bench import KINDS, PLACES, disc  # noqa: E402


def timed(f, dev):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1)


def bits(masks):
    return int(sum(bin(int(x)).count("1") for x in masks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=256)
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
    host = {"clean": frames[idx]}
    damaged = frames[idx].copy()
    for k in range(n):
        cx, cy = PLACES[k % 3]
        disc(damaged[k], cx, cy, 0.19, KINDS[(k // 3 + k) % 3], g)
    host["damaged"] = damaged
    sets = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    groups = torch.empty(n, dtype=torch.int32, device=dev)
    gchunks = torch.empty((n + 1, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    gmasks = torch.empty(n + 1, dtype=torch.int32, device=dev)
    gsizes = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ng = torch.empty(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": mode, "captures": n, "group": 3, "reps": a.reps, "calls_in_flight": a.calls, "whole_batch": {}, "one_per_call": {}}

    def plain_call(fr, k0, m):
        dec.decode_batch_combined_device(fr[k0:k0 + m].data_ptr(), m, chunks[k0:].data_ptr(), masks[k0:].data_ptr(), groups[k0:].data_ptr(),
                                         gchunks[k0:].data_ptr(), gmasks[k0:].data_ptr(), ng.data_ptr(), stream=stream)

    def stream_call(fr, k0, m, flush):
        # (one capture per call: slot k0 and k0 + 1 of the group outputs; the next call overwrites the second, which is zero or its own)
        dec.decode_batch_combined_stream_device(fr[k0:k0 + m].data_ptr(), m, chunks[k0:].data_ptr(), masks[k0:].data_ptr(), groups[k0:].data_ptr(),
                                                gchunks[k0:].data_ptr(), gmasks[k0:].data_ptr(), gsizes[k0:].data_ptr(), ng.data_ptr(), flush=flush,
                                                stream=stream)

    for name, fr in sets.items():
        # (a)
        calls = {"decode_batch_combined": lambda: plain_call(fr, 0, n), "decode_batch_combined_stream": lambda: stream_call(fr, 0, n, True)}
        for f in calls.values():
            f()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                times[k].append(timed(f, dev))
        base, strm = statistics.median(times["decode_batch_combined"]), statistics.median(times["decode_batch_combined_stream"])
        q = statistics.quantiles(times["decode_batch_combined"], n=4)
        res["whole_batch"][name] = {"decode_batch_combined_ms": round(base, 4), "decode_batch_combined_stream_ms": round(strm, 4),
                                    "overhead_pct": round(100.0 * (strm - base) / base, 2),
                                    "baseline_iqr_pct": round(100.0 * (q[2] - q[0]) / base, 2),
                                    "baseline_min_max_ms": [round(min(times["decode_batch_combined"]), 4), round(max(times["decode_batch_combined"]), 4)],
                                    "n_groups": int(ng.item())}
        # (b)
        m = min(a.calls, n - 1)
        per = {"decode_batch_combined": lambda: [plain_call(fr, k, 1) for k in range(m)],
               "decode_batch_combined_stream": lambda: [stream_call(fr, k, 1, k == m - 1) for k in range(m)]}
        for f in per.values():
            f()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in per}
        for _ in range(a.reps):
            for k, f in per.items():
                times[k].append(timed(f, dev))
        res["one_per_call"][name] = {k + "_us_per_capture": round(1000.0 * statistics.median(v) / m, 2) for k, v in times.items()}
    # (c)
    dec.combine_stream_reset()
    fr = host["damaged"]
    alone = plain = strm = full_plain = full_strm = 0
    for k in range(n):
        r = dec.decode_batch_combined(fr[k:k + 1])
        alone += bits(r[2])
        plain += bits(r[5][:r[0]])
        full_plain += int((r[5][:r[0]] == geo.FULL_MASK).sum())
    for k in range(n):
        r = dec.decode_batch_combined_stream(fr[k:k + 1], flush=k == n - 1)
        strm += bits(r[5][:r[0]])
        full_strm += int((r[5][:r[0]] == geo.FULL_MASK).sum())
    res["damaged_one_per_call_chunks"] = {"captures_alone": alone, "decode_batch_combined": plain, "decode_batch_combined_stream": strm,
                                          "complete_groups_plain": full_plain, "complete_groups_stream": full_strm, "frames": nframes,
                                          "chunks_per_frame": geo.CHUNKS_PER_FRAME}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
