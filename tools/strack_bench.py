#!/usr/bin/env python3
"""Device time of ONE source-track launch (vs_strack_launch: one kernel, one wavefront per row) on config 3's lanes
(65536 x 16000 int16), three times over -- a constant track, a vibrato track (F0 +-5 % at 5 Hz) and the vibrato track with
flowgen_shimmer's -n 20 on every row -- and next to them one vs_plan_launch(VS_KIND_SOURCE) of the same lanes on the same
box in the same run, and the time the 2.1 GB of stores take at the HBM rate given.  The vs_ctx timer events bracket each
launch alone (the launch's upload of row records and cos rows included, as it is in a caller's chain); one JSON line
(medians of --reps).

    python tools/strack_bench.py [--lanes 65536] [--reps 5] [--hbm-tbs 8.0]
"""
import argparse
import ctypes as C
import json
import math
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
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n = args.lanes
    hop = int(math.floor(0.010 * fs + 0.5))
    fp = -(-ns // hop)
    f0 = np.array([l.F0 for l in lanes], dtype=np.float32)
    const = (np.float32(fs) / f0).astype(np.int32)
    t = (np.arange(fp) * hop + hop // 2) / float(fs)
    vib = (float(fs) / (f0[:, None].astype(np.float64) * (1.0 + 0.05 * np.sin(2.0 * np.pi * 5.0 * t)[None, :]))).astype(np.int32)
    noisy = (vs.Lane * n)()
    C.memmove(noisy, lanes, C.sizeof(noisy))
    for l in noisy:                       # flowgen_shimmer -n 20: the flag, the linear SNR, the DC flow of .25
        l.flags |= vs.VS_FLAG_NOISE
        l.noise = 100.0
        l.DC = 0.25
    pmin, pmax = fs // 500, -(-fs // 50)      # the range vs_strack_from_pitch gives at the default 50..500 Hz
    rows = vs.strack_rows(n, fp, hop, 0, ns, pmin, pmax)
    cases = (("constant", lanes, np.repeat(const[:, None], fp, axis=1)), ("vibrato", lanes, vib), ("vibrato -n 20", noisy, vib))
    res = {"what": "source track, " + label, "lanes": n, "samples": ns, "frames_per_row": fp,
           "store_gb": round(n * ns * 2 / 1e9, 3), "store_ms_at_hbm_rate": round(n * ns * 2 / (args.hbm_tbs * 1e12) * 1e3, 3)}
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        out_d = dev.room(n * pitch * 2)
        per_d = dev.room(n * fp * 4)
        stat_d = dev.room(n * vs.STRACK_STAT_DTYPE.itemsize)
        ts = []
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            plan.launch(vs.VS_KIND_SOURCE, out_d, pitch)
            eng.timer_mark(1)
            ts.append(eng.timer_elapsed())
        res["vs_plan_launch_source_ms"] = round(float(np.median(ts[1:])), 4)
        ref = dev.get(out_d, (n, pitch))[:, :ns].copy() if n <= 4096 else None
        for name, ln, per in cases:
            eng.dev_upload(per_d, np.ascontiguousarray(per, dtype=np.int32))
            ts = []
            for _ in range(args.reps + 1):
                eng.timer_mark(0)
                eng.source_track_dev(ln, ns, rows, per_d, 4, fp, out_d, pitch, stat_d)
                eng.timer_mark(1)
                ts.append(eng.timer_elapsed())
            st = dev.get(stat_d, (n,), vs.STRACK_STAT_DTYPE)
            key = name.replace(" ", "_").replace("-", "")
            res[key + "_ms"] = round(float(np.median(ts[1:])), 4)
            res[key + "_all_ms"] = [round(v, 4) for v in ts]
            res[key + "_mean_cycles"] = round(float(st["n_cycles"].mean()), 2)
            res[key + "_resets"] = int(st["n_resets"].sum())
            res[key + "_status_or"] = int(np.bitwise_or.reduce(st["status"]))
            if name == "constant" and ref is not None:
                res["constant_equals_vs_source"] = bool(np.array_equal(dev.get(out_d, (n, pitch))[:, :ns], ref))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
