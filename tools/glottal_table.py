#!/usr/bin/env python3
"""The table of README, "glottal": mean OQ, SQ, QOQ and NAQ of 16 of the CPU oracle's vowels (-v a, gain 10, pre-emphasis
1, F0 100, 22050 Hz, seeds 300..315) read on the flow, on the speech inverse-filtered with the known table (de-emphasis
1, scale 1/10) and on the speech itself, with the restatements of tests/ (no device; the device gives the same records
bit for bit, tests/test_gpu_glottal.py).

    python tools/glottal_table.py [--level-open 26] [--level-mid 128]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voice_synth_amd as vs  # noqa: E402
from oracle import pyoracle  # noqa: E402
import glottal_ref as gr  # noqa: E402
import inverse_ref as ir  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level-open", type=int, default=26)
    ap.add_argument("--level-mid", type=int, default=128)
    args = ap.parse_args()
    print("| flowgen args | signal | OQ | SQ | QOQ | NAQ |")
    print("|---|---|---|---|---|---|")
    for fa in ([], ["-s", "5", "-j", "2"], ["-s", "10"]):
        specs = [(["-d", "1", "-f", "100"] + fa, ["-v", "a"], 300 + k) for k in range(16)]
        lanes, d = vs.lanes_from_specs(specs)
        ns = vs.num_samples(22050, d)
        flow, pcm = pyoracle.source(lanes, ns), pyoracle.synth(lanes, ns)
        coefs = np.broadcast_to(vs.vowel_coefficients("a"), (16, 1, 23))
        rows = ir.rows_of(16, 1, 1, 0, ns, 1.0 / lanes[0].gain, lanes[0].pre_emphasis)
        inv, _ = ir.inverse_filter(pcm, coefs, rows, ir.HOLD)
        first = "`%s`" % " ".join(fa) if fa else "(none)"
        for name, x in (("flow", flow), ("inverse-filtered speech", inv), ("speech", pcm)):
            r = gr.measure_and_glottal(x, 22050, args.level_open, args.level_mid)[2]
            print("| %s | %s | %s |" % (first, name, " | ".join("%.4f" % r[f].mean() for f in ("oq", "sq", "qoq", "naq"))))
            first = ""


if __name__ == "__main__":
    main()
