"""Device time of cimbar_hip_rs_decode_erasures (k_rs_erasures) per mode, on blocks already in device memory.

Three block sets per mode, 61 440 blocks each (1 024 mode-68 frames' worth of RS blocks):
  clean       codewords, no erasures (the syndrome pass and nothing else)
  erasures    p - 4 corrupted erasures + 2 errors: the full decode, accepted
  overload    p - 4 erasures + p // 2 further errors: Berlekamp-Massey and Chien run, the block fails or is rejected
Prints one JSON line; --out writes it to a file as well.

    python tools/rs_erasures_bench.py [--blocks 61440] [--reps 20] [--out profiles/r08a_rs_erasures_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libcimbar_amd import decoder as D  # noqa: E402
from tests import rs_cases  # noqa: E402


def block_set(g, n, p, count, kind):
    k = n - p
    code = rs_cases.encode(g.integers(0, 256, (count, k), dtype=np.uint8), p)
    er = np.zeros((count, n), np.uint8)
    counts = np.zeros(count, np.uint8)
    if kind == "clean":
        return code, er, counts
    e = p - 4
    t = 2 if kind == "erasures" else p // 2
    for b in range(count):
        pos = g.permutation(n)
        code[b, pos[:e + t]] ^= g.integers(1, 256, e + t, dtype=np.uint8)
        er[b, :e] = pos[:e]
        counts[b] = e
    return code, er, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=61440)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"blocks": a.blocks, "reps": a.reps, "modes": {}}
    for mode in (68, 67, 66):
        dec = D.HipDecoder(0, mode)
        n, p, k = dec.geo.RS_BLOCK, dec.geo.RS_PARITY, dec.geo.RS_DATA
        g = np.random.default_rng(mode)
        out = {}
        for kind in ("clean", "erasures", "overload"):
            blocks, er, counts = block_set(g, n, p, a.blocks, kind)
            tb, te, tc = (torch.from_numpy(x).to(dev) for x in (blocks, er, counts))
            msgs = torch.empty((a.blocks, k), dtype=torch.uint8, device=dev)
            st = torch.empty(a.blocks, dtype=torch.int8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            run = lambda: dec.rs_decode_erasures_device(tb.data_ptr(), a.blocks, te.data_ptr(), tc.data_ptr(), msgs.data_ptr(), st.data_ptr(), stream)  # noqa: E731
            run()
            torch.cuda.synchronize(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                run()
            t1.record()
            torch.cuda.synchronize(dev)
            ms = t0.elapsed_time(t1) / a.reps
            s = st.cpu().numpy()
            out[kind] = {"ms": round(ms, 4), "ns_per_block": round(ms * 1e6 / a.blocks, 2),
                         "status": {str(v): int((s == v).sum()) for v in (-1, 0, 1)}}
        res["modes"][str(mode)] = out
        dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
