"""Regenerates the table of DESIGN_WIDENING.md "Relaxed flood" from the numpy model of the rule (CPU only, about a minute):

    python tools/relaxed_flood_table.py [--thresholds 12 16]

Mode 68, tests/frames.py distortions of clean_frames(synth, 2, seed=123). Per case and frame: cells whose symbol differs from the clean frame's
under the reference's exact priority flood (co_symbol_pass) and under the relaxed flood at the first threshold, and the rounds at every threshold."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libcimbar_amd import framegen                          # noqa: E402
from tests import frames as F                               # noqa: E402
from tests import relaxed_flood_model as M                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresholds", type=int, nargs="+", default=[12, 16])
    a = ap.parse_args()
    synth = framegen.FrameSynth("cpu")
    _, clean = F.clean_frames(synth, 2, seed=123)
    truth = [M.exact_flood(c)[1] for c in clean]
    rows = {}
    for name, i, frame in M.table_cases(clean):
        plane, wsym = M.exact_flood(frame)
        r = rows.setdefault(name, {"exact": [None, None], "wrong": [None, None], "rounds": {t: [None, None] for t in a.thresholds}})
        r["exact"][i] = int((wsym != truth[i]).sum())
        for t in a.thresholds:
            sym, drift, rounds, dist = M.relaxed_flood(plane, 68, t)
            if t == a.thresholds[0]:
                r["wrong"][i] = int((sym != truth[i]).sum())
            r["rounds"][t][i] = rounds
    t0 = a.thresholds[0]
    print("| case (frame 0 / frame 1) | exact flood wrong | threshold %d wrong | " % t0 + " | ".join("rounds at %d" % t for t in a.thresholds) + " |")
    print("|---" * (3 + len(a.thresholds)) + "|")
    fmt = lambda p: "%s / %s" % tuple(f"{v:,}".replace(",", " ") for v in p)
    for name, r in rows.items():
        print(f"| `{name}` | {fmt(r['exact'])} | {fmt(r['wrong'])} | " + " | ".join(fmt(r["rounds"][t]) for t in a.thresholds) + " |")


if __name__ == "__main__":
    main()
