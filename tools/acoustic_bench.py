#!/usr/bin/env python3
"""Device time of ONE acoustic measurement (vs_measure_launch) of config 3's batch (65536 x 16000 int16, 2.1 GB),
already on the device: synthesised there by Plan.launch(VS_KIND_SYNTH), then measured on the same stream.  The
vs_ctx timer events bracket the measurement alone; one JSON line (median of --reps), with the fraction of a 6.3 TB/s
streaming read the 2 B/sample pass reaches.  Under `rocprofv3 --kernel-trace --stats -- python tools/acoustic_bench.py`
the two kernels appear as vs_ac_period_kernel and vs_ac_marks_kernel.

    python tools/acoustic_bench.py [--lanes 65536] [--reps 5]
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
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n = args.lanes
    plan = eng.plan(lanes, ns)
    pcm_d = eng.dev_alloc(n * pitch * 2)
    out_d = eng.dev_alloc(n * vs.ACOUSTIC_DTYPE.itemsize)
    eng.timer_mark(0)
    plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
    eng.timer_mark(1)
    synth_ms = eng.timer_elapsed()
    times = []
    for _ in range(args.reps + 1):
        eng.timer_mark(0)
        eng.measure_dev(pcm_d, pitch, n, ns, fs, out_d)
        eng.timer_mark(1)
        times.append(eng.timer_elapsed())
    out = eng.dev_download(out_d, (n,), vs.ACOUSTIC_DTYPE)
    plan.close()
    eng.dev_free(pcm_d)
    eng.dev_free(out_d)
    eng.close()
    ms = float(np.median(times[1:]))
    gb = n * ns * 2 / 1e9
    print(json.dumps({"what": "acoustic measurement, " + label, "lanes": n, "samples": ns, "measure_ms": round(ms, 4),
                      "all_ms": [round(t, 4) for t in times], "synth_ms": round(synth_ms, 4),
                      "read_GBps": round(gb / ms * 1e3, 1), "hbm_fraction_of_6.3TBps": round(gb / ms * 1e3 / 6300, 3),
                      "voiced": int((out["status"] == 0).sum()), "mean_jitter_local": float(np.nanmean(out["jitter_local"])),
                      "mean_shimmer_local": float(np.nanmean(out["shimmer_local"])),
                      "mean_hnr_db": float(np.nanmean(out["hnr_db"]))}))


if __name__ == "__main__":
    main()
