"""Device time of a mode-68 decode_batch with colour erasure decoding off, on, and on with damaged frames.

Three cases, 1 024 device-resident frames each (16 rendered frames, or the 12 glare frames of tests/colour_erasure_cases.py, tiled):
  off     clean frames, the setting never touched (nothing new is launched)
  on      clean frames, cimbar_hip_set_colour_erasure_decode(COLOUR_MARGIN_SUGGESTED): one extra launch whose workgroups return at once
  glare   the glare set, setting on: the frames that lack colour chunks are retried
Every case is warmed up, then timed in `rounds` rounds of `reps` calls (device events around the calls); the rounds of the cases alternate, so
a drift of the clock hits all of them. Each library runs in a child process of its own. With --baseline-lib (another build of the same C ABI,
e.g. the parent commit's) that library's `off` time is measured the same way, child processes alternating with this build's, and the result
says whether this build's `off` median lies inside the baseline's own run-to-run spread (min .. max over its rounds).
Prints one JSON line; --out writes it to a file as well.

    python tools/colour_erasure_bench.py [--frames 1024] [--reps 10] [--rounds 6] [--baseline-lib PATH] [--out profiles/colour_erasure_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODE = 68


def worker(lib_path, cases, frames_n, reps, rounds):
    import numpy as np
    import torch
    from libcimbar_amd import decoder as D
    from libcimbar_amd import geometry
    from tests import colour_erasure_cases as K
    geo = geometry.for_mode(MODE)
    lib = ctypes.CDLL(lib_path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.cimbar_hip_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    lib.cimbar_hip_destroy.argtypes = [vp]
    lib.cimbar_hip_destroy.restype = None
    lib.cimbar_hip_decode_batch.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_decode_batch.restype = ctypes.c_int64
    dev = torch.device("cuda", 0)

    def tiled(fr):
        return torch.from_numpy(np.ascontiguousarray(fr[np.arange(frames_n) % len(fr)])).to(dev)

    clean = tiled(K.frames(MODE, 16, 11)[0])
    inputs = {"off": clean, "on": clean}
    if "glare" in cases:
        inputs["glare"] = tiled(K.glare_set(MODE)[0])
    chunks = torch.zeros((frames_n, geo.FRAME_BYTES), dtype=torch.uint8, device=dev)
    masks = torch.zeros(frames_n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctxs, delivered = {}, {}
    for case in cases:
        ctx = vp()
        assert lib.cimbar_hip_create(0, MODE, ctypes.byref(ctx)) == 0
        if case != "off":
            lib.cimbar_hip_set_colour_erasure_decode.argtypes = [vp, i32, i32]
            assert lib.cimbar_hip_set_colour_erasure_decode(ctx, D.COLOUR_MARGIN_SUGGESTED, -1) == 0
        ctxs[case] = ctx

    def run(case):
        rc = lib.cimbar_hip_decode_batch(ctxs[case], vp(inputs[case].data_ptr()), frames_n, D.MEM_DEVICE, 0, 2, vp(chunks.data_ptr()),
                                         vp(masks.data_ptr()), D.MEM_DEVICE, vp(stream) if stream else None)
        assert rc == 0, rc

    for case in cases:                       # warm-up: code objects, scratch growth, the flood scheduler's first look at the batch
        for _ in range(3):
            run(case)
        torch.cuda.synchronize(dev)
        delivered[case] = int(sum(bin(int(m) & 0xFFF).count("1") for m in masks.cpu().numpy()))
    times = {case: [] for case in cases}
    for _ in range(rounds):
        for case in cases:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                run(case)
            t1.record()
            torch.cuda.synchronize(dev)
            times[case].append(t0.elapsed_time(t1) / reps)
    for ctx in ctxs.values():
        lib.cimbar_hip_destroy(ctx)
    print("WORKER " + json.dumps({"times_ms": times, "chunks_delivered": delivered}))


def summary(rounds_ms):
    return {"median_ms": round(statistics.median(rounds_ms), 4), "min_ms": round(min(rounds_ms), 4), "max_ms": round(max(rounds_ms), 4),
            "rounds_ms": [round(t, 4) for t in rounds_ms]}


def child(lib_path, cases, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", lib_path, "--cases", ",".join(cases), "--frames", str(a.frames),
           "--reps", str(a.reps), "--rounds", str(a.rounds)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("WORKER ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--cases", default="off,on,glare")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.cases.split(","), a.frames, a.reps, a.rounds)
        return
    from libcimbar_amd import decoder as D
    this_lib = os.environ.get("CIMBAR_HIP_LIB") or D.LIB_PATH
    res = {"mode": MODE, "frames": a.frames, "reps": a.reps, "rounds_per_process": a.rounds, "colour_margin": D.COLOUR_MARGIN_SUGGESTED}
    mine = {"off": [], "on": [], "glare": []}
    base = []
    delivered = {}
    for k in range(2 if a.baseline_lib else 1):            # baseline, this build, baseline, this build
        if a.baseline_lib:
            base += child(a.baseline_lib, ["off"], a)["times_ms"]["off"]
        w = child(this_lib, ["off", "on", "glare"], a)
        for case in mine:
            mine[case] += w["times_ms"][case]
        delivered = w["chunks_delivered"]
    res["cases"] = {case: summary(t) for case, t in mine.items()}
    res["chunks_delivered"] = delivered
    if a.baseline_lib:
        res["baseline_off"] = summary(base)
        med = res["cases"]["off"]["median_ms"]
        res["off_inside_baseline_spread"] = bool(res["baseline_off"]["min_ms"] <= med <= res["baseline_off"]["max_ms"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
