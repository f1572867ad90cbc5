#!/usr/bin/env python3
"""The figures of README, "vsource": what the source track does in the closed loop pitch track -> source track -> pitch
track -> guided marks on the pitch track's constructed signals, and at the corners of its walk, from the numpy
restatements of tests/ alone (no device).

    python tools/strack_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voice_synth_amd as vs  # noqa: E402

import guided_ref as gr  # noqa: E402
import pitch_ref as pt  # noqa: E402
import pitch_signals as ps  # noqa: E402
import strack_ref as sr  # noqa: E402


def lane_of(args, seed):
    return vs.lane_from_cli(list(args), ["-v", "a"], seed=seed)[0]


def loop(name, x):
    model = pt.track_row(x, 16000)
    r = sr.row_from_pitch(16000, len(x))
    flow, stat, cyc = sr.source_track_one(lane_of(["-c", "0.6", "-a", "8000", "-r", "16000"], 1), len(x), r, model["lag"])
    copy = pt.track_row(flow, 16000)
    vm = (model["lag"] >= r["pmin"]) & (model["lag"] <= r["pmax"])
    vc = (copy["lag"] >= r["pmin"]) & (copy["lag"] <= r["pmax"])
    d = (copy["lag"].astype(int) - model["lag"].astype(int))[vm & vc]
    g = gr.guided_row(flow, 16000, copy)
    print("%-6s %d samples, %d frames: model voiced %d, copy voiced %d, both %d, lag copy - model %+d..%+d; %d cycles, %d "
          "unvoiced samples, %d draws; guided marks of the copy: %d runs, %d marks"
          % (name, len(x), len(model), vm.sum(), vc.sum(), (vm & vc).sum(), d.min(), d.max(), stat["n_cycles"],
             stat["n_unvoiced"], stat["n_draws"], g["guided"][0], len(g["marks"])))


if __name__ == "__main__":
    loop("glide", np.asarray(ps.glide()[0], dtype=np.int16))
    loop("gaps", np.asarray(ps.gaps(), dtype=np.int16))
    flow, stat, cyc = sr.source_track_one(lane_of(["-j", "0.05", "-r", "16000"], 7), 3200, sr.row(4, 730, 0, 3200),
                                          [300, 20, 7, 300])
    print("octave drop 300 -> 20 -> 7 -> 300 at -j 0.05, four frames of 730 samples: %d cycles in 3200 samples, %d resets"
          % (stat["n_cycles"], stat["n_resets"]))
    for mr in (4, 256):
        flow, stat, cyc = sr.source_track_one(lane_of(["-j", "1000", "-r", "16000"], 7), 6000, sr.row(1, 100, 0, 6000), [160],
                                              max_reject=mr)
        print("-j 1000 at P = 160, max_reject %d: %d cycles in 6000 samples, %d resets, %d draws"
              % (mr, stat["n_cycles"], stat["n_resets"], stat["n_draws"]))
