"""The capture path in every capture format, 1080p captures already on the device (one JSON line):

    python tools/capture_formats_bench.py [--n 256] [--reps 10] [--rounds 3] [--out profiles/capture_formats_bench.json]

  preprocess  cimbar_hip_scan_preprocess_fmt              (X1 gray + blur, Otsu, binarize)
  extract     cimbar_hip_extract_batch_fmt                (X1 .. X3, anchor search, X4 warp)
  chain       cimbar_hip_scan_extract_decode_batch_fmt    (extract + decode)

ms per batch of n captures for the nine formats in ONE run, so that NV21 can be read against NV12 and YUYV against NV12 and RGB8 under the same clocks.
The YUV formats (12 / 21 / 420 / 422 / 4221) are timed on both warp routes: a context created with CIMBAR_HIP_WARP_TWOPASS=1 (k_convert_roi in front
of k_warp<3>) and one with =0 (conversion inside k_warp<FMT>); `extract_ms` / `chain_ms` are the default route's, `*_onepass_ms` the other's.
Each figure is the median over `rounds` rounds of `reps` back-to-back calls timed with one event pair; the formats are interleaved inside a round, so a
drift of the clocks hits all of them alike. `spread` is (max - min) / median over the rounds."""
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
from tests import capture_formats as CF                     # noqa: E402
from tests import capture_formats_native as CN              # noqa: E402
from tests import frames as F                               # noqa: E402
from tests.test_oracle_vs_ref import CAMERA_CASES           # noqa: E402

FORMATS = (3, 4, 12, 420, 21, 422, 4221, 30, 40)
YUV = (12, 420, 21, 422, 4221)


def decoder_with_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return D.HipDecoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, n = 1920, 1080, a.n
    synth = framegen.FrameSynth("cpu")
    _, frames = F.clean_frames(synth, len(CAMERA_CASES), seed=90)
    rgbs = [F.camera_frame(frames[k], width=w, height=h, quad=q, background=bg, blur=bl) for k, (bg, q, bl) in enumerate(CAMERA_CASES)]
    dec = {1: decoder_with_env({"CIMBAR_HIP_WARP_TWOPASS": "1"}), 0: decoder_with_env({"CIMBAR_HIP_WARP_TWOPASS": "0"})}
    lib = dec[1]._lib
    d_in = {}
    for fmt in FORMATS:
        base = [(CF.rgb_to_format if fmt in CF.FORMATS else CN.rgb_to_native)(c, fmt) for c in rgbs]
        d_in[fmt] = torch.from_numpy(np.stack([base[k % len(base)] for k in range(n)])).cuda()
    d_bin = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    d_frames = torch.empty((n, 1024, 1024, 3), dtype=torch.uint8, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    d_corners = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    d_chunks = torch.empty((n, 12, 625), dtype=torch.uint8, device="cuda")
    d_masks = torch.empty(n, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def check(ctx, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what}: {rc} {lib.cimbar_hip_last_error(ctx)}")

    def calls(route, fmt):
        ctx = dec[route]._ctx
        return {
            "preprocess": lambda: check(ctx, lib.cimbar_hip_scan_preprocess_fmt(ctx, P(d_in[fmt]), w, h, fmt, n, D.MEM_DEVICE, P(d_bin), None, D.MEM_DEVICE, st), "preprocess"),
            "extract": lambda: check(ctx, lib.cimbar_hip_extract_batch_fmt(ctx, P(d_in[fmt]), w, h, fmt, n, D.MEM_DEVICE, P(d_frames), P(d_status), P(d_corners),
                                                                           D.MEM_DEVICE, st), "extract"),
            "chain": lambda: check(ctx, lib.cimbar_hip_scan_extract_decode_batch_fmt(ctx, P(d_in[fmt]), w, h, fmt, n, D.MEM_DEVICE, 1, 2, P(d_chunks), P(d_masks),
                                                                                      P(d_status), D.MEM_DEVICE, st), "chain"),
        }

    jobs = []                                         # (key, fn)
    for fmt in FORMATS:
        for name, fn in calls(1, fmt).items():
            jobs.append(((fmt, name), fn))
        if fmt in YUV:
            for name, fn in calls(0, fmt).items():
                if name != "preprocess":              # (the route only concerns the warp)
                    jobs.append(((fmt, name + "_onepass"), fn))
    times = {key: [] for key, _ in jobs}
    for _, fn in jobs:                                # warm-up: allocations, the scratch of the two-pass route
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for key, fn in jobs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) / a.reps)
    res = {"n": n, "size": [w, h], "reps": a.reps, "rounds": a.rounds, "default_route": "twopass", "formats": {}}
    for fmt in FORMATS:
        row = {}
        for (f2, name), ts in times.items():
            if f2 != fmt:
                continue
            med = statistics.median(ts)
            row[name + "_ms"] = round(med, 3)
            row[name + "_spread"] = round((max(ts) - min(ts)) / med, 3)
        row["extract_captures_per_s"] = round(n / (row["extract_ms"] / 1e3), 1)
        row["bytes_per_capture"] = int(lib.cimbar_hip_capture_bytes(w, h, fmt))
        res["formats"][str(fmt)] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
