"""Throughput of the lens-undistortion entry points on 1080p RGB captures already on the device (one JSON line):

    python tools/undistort_bench.py [--n 256] [--reps 10]

  calibrate   cimbar_hip_undistort_calibrate_fmt                   (X1 + X2 + anchor search + U1 per capture)
  undistort   cimbar_hip_undistort_batch_fmt, params = NULL         (calibrate + U2 remap, device output)
  remap       cimbar_hip_undistort_batch_fmt, explicit params       (U2 alone, device output): its HBM fraction = bytes moved (capture read +
              RGB written) / time, against 8 TB/s -- an upper bound on the kernel's own time, the call's small host work included
  composite   cimbar_hip_scan_undistort_extract_decode_batch_fmt   (calibrate, remap, extract, decode)
  decode_count  chunks recovered with and without undistortion on a set of barrel-distorted captures (kd 0.002 .. 0.012, four frames each)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libcimbar_amd import decoder as D            # noqa: E402
from tests import distorted_captures as DC        # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    w, h, n = 1920, 1080, a.n
    dec = D.HipDecoder(0)
    lib, ctx = dec._lib, dec._ctx
    base = [DC.case("barrel_1080"), DC.case("pincushion_1080"), DC.case("mild_barrel_1080"), DC.distorted(1920, 1080, 0.006, 12)]
    host = np.stack([base[k % len(base)] for k in range(n)])
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.empty_like(d_in)
    chunks = torch.empty((n, 12, 625), dtype=torch.uint8, device="cuda")
    masks = torch.empty(n, dtype=torch.int32, device="cuda")
    ok = np.zeros(n, np.int32)
    k1 = np.zeros(n, np.float64)
    params = np.array([w // 4, 0, w // 2, 0, h // 4, h // 2, 0, 0, 1, 0.004, 0, 0, 0, 0], np.float64)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def check(rc, what):
        if rc < 0:
            raise RuntimeError(f"{what}: {rc} {lib.cimbar_hip_last_error(ctx)}")

    calls = {
        "calibrate": lambda: check(lib.cimbar_hip_undistort_calibrate_fmt(ctx, P(d_in), w, h, 3, n, D.MEM_DEVICE, ok.ctypes.data, k1.ctypes.data,
                                                                          ctypes.c_void_p(st)), "calibrate"),
        "undistort": lambda: check(lib.cimbar_hip_undistort_batch_fmt(ctx, P(d_in), w, h, 3, n, D.MEM_DEVICE, None, P(d_out), D.MEM_DEVICE, None, None,
                                                                      ctypes.c_void_p(st)), "undistort"),
        "remap": lambda: check(lib.cimbar_hip_undistort_batch_fmt(ctx, P(d_in), w, h, 3, n, D.MEM_DEVICE, params.ctypes.data, P(d_out), D.MEM_DEVICE,
                                                                  None, None, ctypes.c_void_p(st)), "remap"),
        "composite": lambda: check(lib.cimbar_hip_scan_undistort_extract_decode_batch_fmt(ctx, P(d_in), w, h, 3, n, D.MEM_DEVICE, -1, 2, P(chunks), P(masks),
                                                                                          None, None, D.MEM_DEVICE, ctypes.c_void_p(st)), "composite"),
    }
    res = {"n": n, "size": [w, h], "reps": a.reps}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        res[name + "_ms"] = round(ms, 3)
        res[name + "_captures_per_s"] = round(n / (ms / 1e3), 1)
    # decode count: the same barrel-distorted captures through the plain capture path and through the --undistort one
    barrel = np.stack([DC.distorted(w, h, kd, seed) for kd in (0.002, 0.004, 0.006, 0.008, 0.010, 0.012) for seed in (11, 12, 13, 14)])
    dec.reset_ccm()
    _, _, m0, s0 = dec.scan_extract_decode_batch(barrel)
    dec.reset_ccm()
    _, _, m1, s1, uok = dec.scan_undistort_extract_decode_batch(barrel)
    pop = lambda m: int(sum(bin(int(v) & 0xFFF).count("1") for v in m))
    res["decode_count"] = {"captures": len(barrel), "chunks_without_undistort": pop(m0), "chunks_with_undistort": pop(m1),
                           "extracted_without": int((s0 > 0).sum()), "extracted_with": int((s1 > 0).sum()), "calibrated": int(uok.sum())}
    moved = n * w * h * 3 * 2
    res["remap_bytes"] = moved
    res["remap_hbm_fraction"] = round(moved / (res["remap_ms"] / 1e3) / HBM_PEAK, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
