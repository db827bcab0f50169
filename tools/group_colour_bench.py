"""Device time of the group decode's colour vote (cimbar_hip_set_group_colour_vote), mode 68, on captures already in device memory.

1 024 captures in groups of TWO (512 frames rendered by the device encoder, each captured twice), two sets:
  clean     the two captures identical: no group is flagged, the vote's workgroups return at once
  damaged   each capture with a washed, white, black or noise disc (radius 0.09 of the width) at a place the other leaves clean
Per set, decode_batch_combined (device outputs, the groups given) with the setting off and on alternate within one run, `--reps` times each
after a warm-up; the median of the per-call times is reported, with the colour chunks delivered by the captures alone, by plurality groups,
by weighted groups and by weighted groups with the group colour retry. `--lib` times another build of the library (the setting is left
off where that build lacks it): run it once per library, processes alternating, to compare builds. Prints one JSON line; --out writes it
to a file as well.

    python tools/group_colour_bench.py [--n 1024] [--reps 20] [--lib other/libcimbar_hip.so] [--out profiles/group_colour_bench.json]
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

KINDS = ("washed", "white", "washed", "noise", "washed", "black")


def disc(frame, cx, cy, r, kind, g):
    h, w, _ = frame.shape
    yy, xx = np.ogrid[0:h, 0:w]
    d = (yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (r * w) ** 2
    if kind == "white":
        frame[d] = 255
    elif kind == "black":
        frame[d] = 0
    elif kind == "noise":
        frame[d] = g.integers(0, 256, (int(d.sum()), 3), dtype=np.uint8)
    else:
        frame[d] = frame[d].max(axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["CIMBAR_HIP_LIB"] = os.path.abspath(a.lib)
    from libcimbar_amd import decoder as D
    from libcimbar_amd import framegen
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    dec = D.HipDecoder(0, mode)
    has_vote = hasattr(dec._lib, "cimbar_hip_set_group_colour_vote") if a.lib else True
    geo = dec.geo
    nframes = (n + 1) // 2
    payload = framegen.synth_payload(nframes, seed=9, mode=mode).numpy().reshape(nframes, -1)
    frames = dec.encode_batch(payload)
    idx = np.arange(n) // 2
    g = np.random.default_rng(1)
    sets = {"clean": torch.from_numpy(frames[idx]).to(dev)}
    damaged = frames[idx].copy()
    for k in range(n):
        disc(damaged[k], (0.32, 0.68)[k % 2], 0.4 + 0.2 * g.random(), 0.09, KINDS[(k // 2) % len(KINDS)], g)
    sets["damaged"] = torch.from_numpy(damaged).to(dev)
    del damaged
    groups_in = idx.astype(np.int32)
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    groups = torch.empty(n, dtype=torch.int32, device=dev)
    gchunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    gmasks = torch.empty(n, dtype=torch.int32, device=dev)
    ng = torch.empty(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    symc = geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)
    colour = lambda m: int(sum(bin(int(x) >> symc).count("1") for x in m))
    res = {"mode": mode, "captures": n, "group": 2, "reps": a.reps, "lib": a.lib or "libcimbar_hip.so", "has_vote": bool(has_vote), "sets": {}}

    def call(fr):
        dec.decode_batch_combined_device(fr.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), groups.data_ptr(), gchunks.data_ptr(), gmasks.data_ptr(),
                                         ng.data_ptr(), groups=groups_in, stream=stream)

    def setting(vote, retry=False):
        if has_vote:
            dec.set_group_colour_vote(vote)
            dec.set_colour_erasure_decode(D.COLOUR_MARGIN_SUGGESTED if retry else 0)

    for name, fr in sets.items():
        variants = ["off", "on"] if has_vote else ["off"]
        for v in variants:
            setting(v == "on")
            call(fr)
        torch.cuda.synchronize(dev)
        times = {v: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                setting(v == "on")
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(fr)
                t1.record()
                torch.cuda.synchronize(dev)
                times[v].append(t0.elapsed_time(t1))
        row = {f"{v}_ms": round(statistics.median(times[v]), 4) for v in variants}
        row.update({f"{v}_min_max_ms": [round(min(times[v]), 4), round(max(times[v]), 4)] for v in variants})
        if has_vote:
            row["overhead_pct"] = round(100.0 * (row["on_ms"] - row["off_ms"]) / row["off_ms"], 2)
            counts = {}
            for label, vote, retry in (("plurality_groups", False, False), ("weighted_groups", True, False), ("weighted_groups_retry", True, True)):
                setting(vote, retry)
                call(fr)
                torch.cuda.synchronize(dev)
                gm = gmasks.cpu().numpy().view(np.uint32)[:int(ng.item())]
                counts[label] = colour(gm)
                if label == "plurality_groups":
                    counts["captures_alone"] = colour(np.bitwise_or.reduce(masks.cpu().numpy().view(np.uint32).reshape(-1, 2), axis=1)) if n % 2 == 0 else None
            row["colour_chunks"] = counts
            row["colour_chunks_total"] = int(ng.item()) * (geo.CHUNKS_PER_FRAME - symc)
            setting(False)
        res["sets"][name] = row
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
