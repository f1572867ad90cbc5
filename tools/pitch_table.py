#!/usr/bin/env python3
"""The figures of README, "pitch", from the numpy restatements of tests/ alone (no device): what the path does on the
constructed signals of tests/pitch_signals.py and on the first-pass residuals of the 16 oracle vowels (`-d 1 -f 100`,
`-v a`, 22050 Hz, seeds 300..315; first pass as tests/cplpc_ref.py runs it, de-emphasis 1, scale 1/gain, f0_min 50).

    python tools/pitch_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voice_synth_amd as vs  # noqa: E402
from oracle import pyoracle  # noqa: E402

import acoustic_ref as ar  # noqa: E402
import cplpc_ref as cp  # noqa: E402
import pitch_ref as pr  # noqa: E402
import pitch_signals as ps  # noqa: E402


def cands_of(r):
    return list(zip(r["cand_lag"][:r["n_cand"]].tolist(), r["cand_q"][:r["n_cand"]].tolist()))


def line(name, rec, fs):
    s = pr.summary(rec, fs)
    greedy = [pr.greedy(cands_of(r)) for r in rec]
    differ = sum(1 for g, r in zip(greedy, rec) if g != int(r["lag"]))
    lags = rec["lag"][rec["lag"] > 0]
    print("%-28s frames %3d voiced %3d segments %d lags %s..%s, greedy pick differs in %d frames" % (
        name, s["frames"], s["voiced"], s["segments"], lags.min() if len(lags) else "-", lags.max() if len(lags) else "-",
        differ))


def oracle(args):
    specs = [(["-d", "1", "-f", "100"] + list(args), ["-v", "a"], 300 + k) for k in range(16)]
    lanes, d = vs.lanes_from_specs(specs)
    pcm = pyoracle.synth(lanes, vs.num_samples(22050, d))
    first = cp.first_pass(pcm, 22050, scale=1.0 / lanes[0].gain, first_de_emphasis=1.0)
    rec, nfr = pr.track(first["residual"], 22050)
    return first, rec, nfr


if __name__ == "__main__":
    print("smallest distance of 256*log2(t) to a rounding tie, t <= 2048: %.2e" % pr.log2_margin())
    x, peaks, periods = ps.glide()
    line("glide 220 -> 80", pr.track_row(x, 16000), 16000)
    print("    vs_measure's restatement on the same row: p0 %d" % ar.measure_row(x, 16000)[0]["p0"])
    line("train, zeros, noise, train", pr.track_row(ps.gaps(), 16000), 16000)
    line("octave trap (P 160)", pr.track_row(ps.octave_trap(), 16000), 16000)
    line("subharmonic, octave_q 328", pr.track_row(ps.subharmonic(), 16000), 16000)
    line("subharmonic, octave_q 3277", pr.track_row(ps.subharmonic(), 16000, octave_q=3277), 16000)
    for args in (("-s", "10"), ("-s", "2", "-n", "20")):
        first, rec, nfr = oracle(args)
        print("oracle vowels %s: vs_measure p0 %s" % (" ".join(args), sorted(set(first["meas"]["p0"].tolist()))))
        for i in (0, 6):
            line("    row %d" % i, rec[i, :nfr[i]], 22050)
        allr = np.concatenate([rec[i, :nfr[i]] for i in range(16)])
        inside = (allr["lag"] >= 215) & (allr["lag"] <= 225)
        print("    all 16 rows: %d frames, %d within lags 215..225, %d unvoiced" % (len(allr), inside.sum(),
                                                                                  (allr["lag"] == 0).sum()))
