#!/usr/bin/env python3
"""Device time of ONE pitch track (vs_pitch_launch: the candidate kernel and the path kernel) of config 3's batch
(65536 x 16000 int16 at 16 kHz: tmax 320, 291 lags, 94 frames a row), already on the device, and next to it one
vs_measure_launch of the same batch on the same box.  The vs_ctx timer events bracket each launch alone; one JSON line
(medians of --reps), with the candidate kernel's share of the fp64 vector FMA rate when --split gives its time.  The split
between the two kernels comes from `rocprofv3 --kernel-trace --stats -- python tools/pitch_bench.py`, where they appear
as vs_pt_cand_kernel and vs_pt_path_kernel.

    python tools/pitch_bench.py [--lanes 65536] [--reps 5] [--hop-ms 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voice_synth_amd as vs  # noqa: E402
from voice_synth_amd import configs  # noqa: E402

FMA_PEAK = 256 * 4 * 16 * 2.4e9   # CUs x SIMDs x fp64 FMA lanes a cycle x Hz: 39.3e12 FMAs/s, the vector peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hop-ms", type=float, default=10.0)
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n = args.lanes
    hop_s = args.hop_ms / 1000.0
    fp = max(1, vs.pitch_frames(fs, ns, hop_s=hop_s))
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        fr_d = dev.room(n * fp * vs.PITCH_FRAME_DTYPE.itemsize)
        out_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        track, measure = [], []
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            eng.pitch_dev(pcm_d, pitch, n, ns, fs, fp, fr_d, hop_s=hop_s)
            eng.timer_mark(1)
            track.append(eng.timer_elapsed())
            eng.timer_mark(0)
            eng.measure_dev(pcm_d, pitch, n, ns, fs, out_d)
            eng.timer_mark(1)
            measure.append(eng.timer_elapsed())
        head = dev.get(fr_d, (min(n, 256), fp), vs.PITCH_FRAME_DTYPE)
    eng.close()
    tmax = int(np.ceil(fs / 50.0))
    tmin = int(np.floor(fs / 500.0))
    fmas = float(n) * fp * (2 * tmax) * (tmax + 3 - tmin)
    ms = float(np.median(track[1:]))
    print(json.dumps({"what": "pitch track, " + label, "lanes": n, "samples": ns, "frames_per_row": fp,
                      "pitch_ms": round(ms, 4), "all_ms": [round(t, 4) for t in track],
                      "measure_ms": round(float(np.median(measure[1:])), 4), "fma_count": fmas,
                      "ms_at_fp64_vector_peak": round(fmas / FMA_PEAK * 1e3, 2),
                      "both_kernels_share_of_peak": round(fmas / FMA_PEAK * 1e3 / ms, 3),
                      "voiced_frames_of_first_rows": int((head["lag"] > 0).sum()), "frames_of_first_rows": int(head.size)}))


if __name__ == "__main__":
    main()
