"""Captures per second of mode auto-detection (cimbar_hip_auto_scan_extract_decode_batch_fmt) on 1080p NV12 batches already in device memory.

  a  per_mode        the per-mode entry point (cimbar_hip_scan_extract_decode_batch_fmt) in the captures' own mode (68)
  b  auto_right_first auto, candidates [68, 66, 67, 4]: every capture accepted in the first phase
  c  auto_right_last  auto, the web receiver's [66, 68, 67, 4] on mode-4 captures: every capture goes through all four phases
  d  auto_no_match    auto, candidates [66, 67] on mode-68 captures: two full phases, nothing accepted
  e  shim_auto        libcimbar_recv_hip.so's cimbard_hip_scan_extract_decode_auto, one host capture per call
`--n` captures per batch (a few distinct ones, rendered on the host, repeated); per case one warm-up call, then the median of `--reps` calls.
Prints one JSON line; --out writes it to a file as well. --case picks one case (for a kernel trace of it).

    python tools/automode_bench.py [--n 1024] [--reps 3] [--case c] [--out profiles/automode_bench.json]
"""
import argparse
import ctypes
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
from tests import automode_model as AM  # noqa: E402
from tests import capture_formats as CF  # noqa: E402

W, H, FMT = 1920, 1080, 12
DISTINCT = 8


def batch(mode, n):
    caps = [CF.rgb_to_format(AM.capture(mode, 40 + k), FMT).reshape(-1) for k in range(DISTINCT)]
    return torch.from_numpy(np.stack([caps[f % DISTINCT] for f in range(n)])).cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", default="abcde")
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    res = {"metric": "captures/s, 1080p NV12, mode auto-detection", "n": n, "reps": args.reps, "cases": {}}
    outs = {}

    def out(slot):
        if slot not in outs:
            outs[slot] = (torch.zeros((n, slot), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
                          torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
        return outs[slot]

    def record(name, sec, total, extra=None):
        res["cases"][name] = {"captures_per_s": round(n / sec, 1) if name != "e_shim_auto" else round(1 / sec, 1), "ms_per_call": round(sec * 1e3, 3),
                              "good_bytes": int(total), **(extra or {})}

    if "a" in args.case:
        src = batch(68, n)
        dec = D.HipDecoder(0, 68)
        ch, mk, _, stt = out(dec.geo.CHUNK * dec.geo.CHUNKS_PER_FRAME)
        lib = dec._lib

        def run_a():
            return lib.cimbar_hip_scan_extract_decode_batch_fmt(dec._ctx, ctypes.c_void_p(src.data_ptr()), W, H, FMT, n, D.MEM_DEVICE, 1, 2,
                                                                ctypes.c_void_p(ch.data_ptr()), ctypes.c_void_p(mk.data_ptr()),
                                                                ctypes.c_void_p(stt.data_ptr()), D.MEM_DEVICE, None)
        record("a_per_mode", timed(run_a, args.reps), int((mk.cpu().numpy().view(np.uint32) == 0xFFF).sum()) * 7500)
        dec.close()
        del src
    for case, mode, order in (("b", 68, [68, 66, 67, 4]), ("c", 4, [66, 68, 67, 4]), ("d", 68, [66, 67])):
        if case not in args.case:
            continue
        src = batch(mode, n)
        dec = D.AutoDecoder(0, order)
        sl, mk, md, stt = out(dec.slot)
        last = {}

        def run():
            last["t"] = dec.scan_extract_decode_device(src.data_ptr(), W, H, n, sl.data_ptr(), mk.data_ptr(), md.data_ptr(), stt.data_ptr(), preprocess=1, fmt=FMT)
        sec = timed(run, args.reps)
        modes = md.cpu().numpy()
        record({"b": "b_auto_right_first", "c": "c_auto_right_last", "d": "d_auto_no_match"}[case], sec, last["t"],
               {"order": order, "accepted": {int(m): int((modes == m).sum()) for m in np.unique(modes)}})
        dec.close()
        del src
    if "e" in args.case:
        lib = ctypes.CDLL(os.path.join(ROOT, "libcimbar_amd", "libcimbar_recv_hip.so"))
        caps = [np.ascontiguousarray(CF.rgb_to_format(AM.capture(4, 40 + k), FMT).reshape(-1)) for k in range(DISTINCT)]
        buf = np.zeros(7500, np.uint8)
        mode = ctypes.c_int(0)
        got = {}

        def run_e(k=[0]):
            c = caps[k[0] % DISTINCT]
            k[0] += 1
            got["r"] = lib.cimbard_hip_scan_extract_decode_auto(c.ctypes.data_as(ctypes.c_void_p), W, H, FMT, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                                                ctypes.byref(mode))
        record("e_shim_auto", timed(run_e, max(args.reps, 16)), got["r"], {"mode": mode.value, "note": "mode-4 captures, [66, 68, 67, 4]: calls/s"})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
