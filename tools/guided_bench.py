#!/usr/bin/env python3
"""Device time of ONE guided measurement (vs_guided_launch: the plan kernel and the walk kernel) of config 3's batch
(65536 x 16000 int16 at 16 kHz: 94 frames a row), already on the device behind one vs_pitch_launch, and next to it one
vs_pitch_launch and one vs_measure_launch of the same batch on the same box.  The vs_ctx timer events bracket each launch
alone; one JSON line (medians of --reps).  The split between the kernels comes from `rocprofv3 --kernel-trace --stats --
python tools/guided_bench.py`, where they appear as vs_mg_plan_kernel and vs_mg_walk_kernel beside vs_ac_marks_kernel
(the walk kernel streams the same PCM once, as that one does) and the two pitch kernels.

    python tools/guided_bench.py [--lanes 65536] [--reps 5] [--longest]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--longest", action="store_true")
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n = args.lanes
    fp = max(1, vs.guided_plan(fs, ns)["n_frames"])
    mp = 256
    seg = vs.VS_MG_LONGEST if args.longest else vs.VS_MG_ALL
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        fr_d = dev.room(n * fp * vs.PITCH_FRAME_DTYPE.itemsize)
        out_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        out2_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        rec_d = dev.room(n * vs.GUIDED_REC_DTYPE.itemsize)
        mk_d = dev.room(n * mp * 4)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        track, guided, measure = [], [], []
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            eng.pitch_dev(pcm_d, pitch, n, ns, fs, fp, fr_d)
            eng.timer_mark(1)
            track.append(eng.timer_elapsed())
            eng.timer_mark(0)
            eng.measure_guided_dev(pcm_d, pitch, n, ns, fs, fr_d, fp, out_d, rec_d, mk_d, mp, segments=seg)
            eng.timer_mark(1)
            guided.append(eng.timer_elapsed())
            eng.timer_mark(0)
            eng.measure_dev(pcm_d, pitch, n, ns, fs, out2_d, marks_ptr=mk_d, marks_pitch=mp)
            eng.timer_mark(1)
            measure.append(eng.timer_elapsed())
        got = dev.get(out_d, (n,), vs.ACOUSTIC_DTYPE)
        rec = dev.get(rec_d, (n,), vs.GUIDED_REC_DTYPE)
        plain = dev.get(out2_d, (n,), vs.ACOUSTIC_DTYPE)
    eng.close()
    med = lambda v: round(float(np.median(v[1:])), 4)  # noqa: E731
    print(json.dumps({"what": "guided marks, " + label, "lanes": n, "samples": ns, "frames_per_row": fp,
                      "segments": "longest" if args.longest else "all", "guided_ms": med(guided),
                      "all_ms": [round(t, 4) for t in guided], "pitch_ms": med(track), "measure_ms": med(measure),
                      "rows_status_0": int((got["status"] == 0).sum()), "rows_status_0_measure": int((plain["status"] == 0).sum()),
                      "mean_segments": round(float(rec["n_segments"].mean()), 3),
                      "mean_frames_walked": round(float(rec["n_frames_walked"].mean()), 2),
                      "mean_periods": round(float(got["n_periods"].mean()), 2),
                      "mean_periods_measure": round(float(plain["n_periods"].mean()), 2)}))


if __name__ == "__main__":
    main()
