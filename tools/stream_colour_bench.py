"""Device time of the stream calls with their colour vote (cimbar_hip_set_stream_colour_vote) off and on, mode 68, captures already in device memory.

Sets of 1 024 captures: `clean` and `damaged` are tools/combine_stream_bench.py's (groups of three; a disc of radius 0.19 per capture at a place
the other two leave clean), `washed` is the damaged set of tools/group_colour_bench.py (groups of two; a washed, white, noise or black disc of
radius 0.09 of the width per capture, disjoint within a group). Per set, the setting off and on alternating within one run (a
combine_stream_reset outside the timed region between them), medians of `--reps`:
  (a) one stream call over all n captures with a flush, device outputs
  (b) one capture per call, `--calls` calls in flight on one stream and one synchronise at the end: time per capture
`--recovery`: the washed set fed as n calls of one capture with the setting on (host outputs); the groups' masks and chunks must equal those
of ONE decode_batch_combined call with cimbar_hip_set_group_colour_vote on -- a condition, the run fails otherwise -- and the colour chunks
are counted against the same stream fed with the setting off.
`--lib` times another build of the library (the setting stays off where that build lacks it): run it once per library, processes
alternating, to compare builds. Prints one JSON line; --out writes it to a file as well.

    python tools/stream_colour_bench.py [--n 1024] [--reps 20] [--calls 256] [--sets clean,damaged,washed] [--recovery] [--lib other.so] [--out x.json]
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


def timed(f, dev):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    f()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=256)
    ap.add_argument("--sets", default="clean,damaged,washed")
    ap.add_argument("--recovery", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["CIMBAR_HIP_LIB"] = os.path.abspath(a.lib)
    from libcimbar_amd import decoder as D
    from libcimbar_amd import framegen
    from tools import combine_bench as CB
    from tools import group_colour_bench as GB
    dev = torch.device("cuda", 0)
    mode, n = 68, a.n
    dec = D.HipDecoder(0, mode)
    has_vote = hasattr(dec._lib, "cimbar_hip_set_stream_colour_vote")
    geo = dec.geo
    wanted = [s for s in a.sets.split(",") if s]
    host = {}
    g = np.random.default_rng(1)
    if "clean" in wanted or "damaged" in wanted:
        nframes = (n + 2) // 3
        frames = dec.encode_batch(framegen.synth_payload(nframes, seed=9, mode=mode).numpy().reshape(nframes, -1))
        idx = np.arange(n) // 3
        if "clean" in wanted:
            host["clean"] = frames[idx]
        if "damaged" in wanted:
            damaged = frames[idx].copy()
            for k in range(n):
                cx, cy = CB.PLACES[k % 3]
                CB.disc(damaged[k], cx, cy, 0.19, CB.KINDS[(k // 3 + k) % 3], g)
            host["damaged"] = damaged
    if "washed" in wanted or a.recovery:
        nframes = (n + 1) // 2
        frames = dec.encode_batch(framegen.synth_payload(nframes, seed=9, mode=mode).numpy().reshape(nframes, -1))
        washed = frames[np.arange(n) // 2].copy()
        g2 = np.random.default_rng(1)
        for k in range(n):
            GB.disc(washed[k], (0.32, 0.68)[k % 2], 0.4 + 0.2 * g2.random(), 0.09, GB.KINDS[(k // 2) % len(GB.KINDS)], g2)
        host["washed"] = washed
    chunks = torch.empty((n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.empty(n, dtype=torch.int32, device=dev)
    groups = torch.empty(n, dtype=torch.int32, device=dev)
    gchunks = torch.empty((n + 1, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    gmasks = torch.empty(n + 1, dtype=torch.int32, device=dev)
    gsizes = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ng = torch.empty(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"mode": mode, "captures": n, "reps": a.reps, "calls_in_flight": a.calls, "lib": a.lib or "libcimbar_hip.so", "has_stream_vote": bool(has_vote),
           "sets": {}}
    variants = ["off", "on"] if has_vote else ["off"]

    def setting(v):
        torch.cuda.synchronize(dev)
        dec.combine_stream_reset()
        if has_vote:
            dec.set_stream_colour_vote(v == "on")

    def stream_call(fr, k0, m, flush):
        dec.decode_batch_combined_stream_device(fr[k0:k0 + m].data_ptr(), m, chunks[k0:].data_ptr(), masks[k0:].data_ptr(), groups[k0:].data_ptr(),
                                                gchunks[k0:].data_ptr(), gmasks[k0:].data_ptr(), gsizes[k0:].data_ptr(), ng.data_ptr(), flush=flush,
                                                stream=stream)

    symc = geo.SYM_BLOCKS // (geo.CHUNK // geo.RS_DATA)
    colour = lambda m: int(sum(bin(int(x) >> symc).count("1") for x in m))
    for name in wanted:
        fr = torch.from_numpy(host[name]).to(dev)
        m = min(a.calls, n - 1)
        # a damaged capture alone in a call takes the exact flood replay, about 10 ms: fewer repetitions of (b) there
        reps_b = a.reps if name == "clean" else max(3, a.reps // 5)
        whole = lambda: stream_call(fr, 0, n, True)
        single = lambda: [stream_call(fr, k, 1, k == m - 1) for k in range(m)]
        row = {}
        for label, f, reps, scale in (("whole_batch_ms", whole, a.reps, 1.0), ("one_per_call_us_per_capture", single, reps_b, 1000.0 / m)):
            for v in variants:
                setting(v)
                f()
            times = {v: [] for v in variants}
            for _ in range(reps):
                for v in variants:
                    setting(v)
                    times[v].append(timed(f, dev) * scale)
            row[label] = {v: round(statistics.median(times[v]), 4) for v in variants}
            row[label + "_min_max"] = {v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in variants}
        res["sets"][name] = row
        del fr
    if a.recovery and has_vote:
        fr = host["washed"]
        ref = D.HipDecoder(0, mode)
        ref.set_group_colour_vote(True)
        want_ng, _, _, _, want_chunks, want_masks = ref.decode_batch_combined(fr)
        ref.close()
        counts = {}
        for v in ("off", "on"):
            setting(v)
            got_masks, got_chunks = [], []
            for k in range(n):
                r = dec.decode_batch_combined_stream(fr[k:k + 1], flush=k == n - 1)
                got_masks += r[5][:r[0]].tolist()
                got_chunks += list(r[4][:r[0]])
            counts[v] = colour(got_masks)
            if v == "on":
                same = got_masks == want_masks[:want_ng].tolist() and bool((np.stack(got_chunks) == want_chunks[:want_ng]).all())
        res["recovery"] = {"groups": int(want_ng), "colour_chunks_total": int(want_ng) * (geo.CHUNKS_PER_FRAME - symc),
                           "one_call_plain_vote_on": colour(want_masks[:want_ng]), "stream_one_per_call_vote_off": counts["off"],
                           "stream_one_per_call_vote_on": counts["on"], "equal_to_one_call": bool(same)}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.recovery and has_vote and not res["recovery"]["equal_to_one_call"]:
        sys.exit("the stream calls with the vote on do not deliver what the one-call plain vote-on run delivers")


if __name__ == "__main__":
    main()
