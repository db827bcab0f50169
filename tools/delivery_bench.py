"""Device and wall time of chunk delivery (cimbar_hip_deliver_chunks) beside the decode it follows, mode 68.

1 024 device-resident frames rendered from a fountain-shaped payload (consecutive block ids), in two sets: `distinct` (1 024 different frames) and
`thrice` (342 different frames, each present three times in a row -- a camera that sees every displayed frame three times). The slots and masks the
delivery call reads are those a real decode_batch of the set wrote.
  (a) the delivery call alone, device outputs, device events around `reps` calls: flags 0, DEDUP | DROP_EMPTY, and REMEMBER | DROP_EMPTY twice --
      `remember_seen` (every header already remembered: the steady state of a repeated batch, nothing is copied) and `remember_fresh` (the table
      emptied before every call, outside the timed window, so every call looks up, delivers and records: one call per window)
  (b) today's path: decode_batch, then all slots and all masks copied to page-locked host memory
  (c) decode_batch, the delivery call (DEDUP | DROP_EMPTY), the count copied to the host, then count * chunk_size bytes
      (b) and (c) are host-clock times around work that ends in a synchronise; `decode` is decode_batch alone, the same way
Every case is warmed up; the cases alternate inside each round, so a drift of the clock hits all of them; medians over the rounds.
Prints one JSON line; --out writes it to a file as well.

    python tools/delivery_bench.py [--frames 1024] [--reps 20] [--rounds 7] [--out profiles/delivery_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODE = 68


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from libcimbar_amd import HipDecoder, framegen
    from libcimbar_amd import decoder as D
    assert torch.cuda.is_available(), "delivery_bench needs a GPU"
    dev = torch.device("cuda", 0)
    dec = HipDecoder(0, MODE)
    geo = dec.geo
    n, per, cs = a.frames, geo.CHUNKS_PER_FRAME, geo.CHUNK
    st = torch.cuda.current_stream(dev).cuda_stream
    payload = framegen.synth_payload(n, seed=5).numpy().reshape(n, per * cs)
    sets = {"distinct": np.arange(n), "thrice": np.arange(n) // 3}
    res = {"mode": MODE, "frames": n, "reps": a.reps, "rounds": a.rounds, "sets": {}}
    h_chunks = torch.empty((n, per * cs), dtype=torch.uint8).pin_memory()
    h_masks = torch.empty((n,), dtype=torch.int32).pin_memory()
    h_packed = torch.empty((n * per * cs,), dtype=torch.uint8).pin_memory()
    h_count = torch.empty((1,), dtype=torch.int32).pin_memory()
    frames = torch.empty((n,) + tuple(geo.FRAME_SHAPE), dtype=torch.uint8, device=dev)
    chunks = torch.zeros((n, per * cs), dtype=torch.uint8, device=dev)
    masks = torch.zeros((n,), dtype=torch.int32, device=dev)
    packed = torch.zeros((n * per * cs,), dtype=torch.uint8, device=dev)
    src = torch.zeros((n * per,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    ALL = D.DELIVER_DEDUP | D.DELIVER_DROP_EMPTY
    REM = D.DELIVER_REMEMBER | D.DELIVER_DROP_EMPTY

    def decode():
        dec.decode_batch_device(frames.data_ptr(), n, chunks.data_ptr(), masks.data_ptr(), False, 2, st)

    def deliver(flags):
        dec.deliver_chunks_device(chunks.data_ptr(), masks.data_ptr(), n, packed.data_ptr(), src.data_ptr(), count.data_ptr(), stream=st, flags=flags)

    def events(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / reps

    def wall(fn, reps):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) * 1e3 / reps

    def path_b():
        decode()
        h_chunks.copy_(chunks, non_blocking=True)
        h_masks.copy_(masks, non_blocking=True)
        torch.cuda.synchronize(dev)

    def path_c():
        decode()
        deliver(ALL)
        h_count.copy_(count, non_blocking=True)
        torch.cuda.synchronize(dev)
        k = int(h_count[0]) * cs
        h_packed[:k].copy_(packed[:k], non_blocking=True)
        torch.cuda.synchronize(dev)

    def decode_sync():
        decode()
        torch.cuda.synchronize(dev)

    def fresh():
        dec.delivery_reset()
        return events(lambda: deliver(REM), 1)

    for name, idx in sets.items():
        pl = torch.from_numpy(np.ascontiguousarray(payload[idx])).to(dev)
        dec.encode_batch_device(pl.data_ptr(), n, frames.data_ptr(), st)
        dec.reset_ccm()
        decode()
        torch.cuda.synchronize(dev)
        assert bool((chunks == pl).all()) and bool((masks == 0xFFF).all())
        counts = {}
        for key, flags in (("flags0", 0), ("dedup_drop_empty", ALL)):
            deliver(flags)
            torch.cuda.synchronize(dev)
            counts[key] = int(count.cpu()[0])
        assert counts["flags0"] == n * per and counts["dedup_drop_empty"] == len(set(idx.tolist())) * per
        dec.delivery_reset()
        cases = {
            "deliver_flags0": lambda: events(lambda: deliver(0), a.reps),
            "deliver_dedup_drop_empty": lambda: events(lambda: deliver(ALL), a.reps),
            "deliver_remember_seen": lambda: events(lambda: deliver(REM), a.reps),
            "deliver_remember_fresh": lambda: statistics.median(fresh() for _ in range(a.reps)),
            "decode": lambda: wall(decode_sync, a.reps),
            "b_decode_copy_all_slots": lambda: wall(path_b, a.reps),
            "c_decode_deliver_copy_packed": lambda: wall(path_c, a.reps),
        }
        for fn in cases.values():            # warm-up: code objects, scratch growth, the table, the page-locked copies
            fn()
        times = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, fn in cases.items():
                if k == "deliver_remember_seen":
                    deliver(REM)             # (the fresh case before it left the table as one call fills it; make sure)
                times[k].append(fn())
        out = {k: summary(v) for k, v in times.items()}
        out["chunks_delivered"] = counts
        out["bytes_to_host"] = {"b": n * per * cs + 4 * n, "c": counts["dedup_drop_empty"] * cs + 4}
        out["c_over_b"] = round(out["c_decode_deliver_copy_packed"]["median_ms"] / out["b_decode_copy_all_slots"]["median_ms"], 4)
        res["sets"][name] = out
    res["stats_after"] = list(dec.delivery_stats())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
