#!/usr/bin/env python3
"""Device time of ONE PSOLA launch (vs_psola_launch: the plan kernel and the overlap-add kernel) of config 3's batch
(65536 x 16000 int16 at 16 kHz), already on the device, with the marks of one vs_guided_launch (VS_MG_ALL) behind one
vs_pitch_launch and, as the target, the cycle log of one vs_strack_launch on a vibrato track (F0 +-5 % at 5 Hz, the lanes'
own jitter), read in place at strides 32 / 24.  The vs_ctx timer events bracket each launch alone; one JSON line (medians
of --reps) with the time the 6 bytes a sample (two int16 reads, one store) take at the HBM rate given.  The split between
the two kernels comes from `rocprofv3 --kernel-trace --stats -- python tools/psola_bench.py`, where they appear as
vs_ps_plan_kernel and vs_ps_ola_kernel beside vs_mg_plan_kernel and vs_mg_walk_kernel.

    python tools/psola_bench.py [--lanes 65536] [--reps 5] [--hbm-tbs 8.0]
"""
import argparse
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
    gp = vs.guided_plan(fs, ns)
    fp = max(1, gp["n_frames"])
    mp, sgp, cp, sp = 256, 4, 256, 256
    hop = int(math.floor(0.010 * fs + 0.5))
    tfp = -(-ns // hop)
    f0 = np.array([l.F0 for l in lanes], dtype=np.float64)
    t = (np.arange(tfp) * hop + hop // 2) / float(fs)
    vib = (float(fs) / (f0[:, None] * (1.0 + 0.05 * np.sin(2.0 * np.pi * 5.0 * t)[None, :]))).astype(np.int32)
    rows = vs.strack_rows(n, tfp, hop, 0, ns, gp["tmin"], gp["tmax"])
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        out_d = dev.room(n * pitch * 2)
        flow_d = dev.room(n * pitch * 2)
        fr_d = dev.room(n * fp * vs.PITCH_FRAME_DTYPE.itemsize)
        meas_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        rec_d = dev.room(n * vs.GUIDED_REC_DTYPE.itemsize)
        mk_d = dev.room(n * mp * 4)
        sg_d = dev.room(n * sgp * vs.GUIDED_SEG_DTYPE.itemsize)
        per_d = dev.put(vib)
        sst_d = dev.room(n * vs.STRACK_STAT_DTYPE.itemsize)
        cyc_d = dev.room(n * cp * vs.STRACK_CYCLE_DTYPE.itemsize)
        stat_d = dev.room(n * vs.PSOLA_STAT_DTYPE.itemsize)
        sy_d = dev.room(n * sp * vs.PSOLA_MARK_DTYPE.itemsize)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        eng.pitch_dev(pcm_d, pitch, n, ns, fs, fp, fr_d)
        guided, strack, psola = [], [], []
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            eng.measure_guided_dev(pcm_d, pitch, n, ns, fs, fr_d, fp, meas_d, rec_d, mk_d, mp, sg_d, sgp)
            eng.timer_mark(1)
            guided.append(eng.timer_elapsed())
            eng.timer_mark(0)
            eng.source_track_dev(lanes, ns, rows, per_d, 4, tfp, flow_d, pitch, sst_d, cycles_ptr=cyc_d, cycles_pitch=cp)
            eng.timer_mark(1)
            strack.append(eng.timer_elapsed())
            eng.timer_mark(0)
            eng.psola_dev(pcm_d, pitch, n, ns, mk_d, mp, rec_d, cyc_d, 32, cyc_d + 4, 32, sst_d + 4, 24, cp, out_d, pitch,
                          stat_d, sy_d, sp, segs_ptr=sg_d, seg_pitch=sgp, pmin=gp["tmin"], pmax=gp["tmax"])
            eng.timer_mark(1)
            psola.append(eng.timer_elapsed())
        st = dev.get(stat_d, (n,), vs.PSOLA_STAT_DTYPE)
        rec = dev.get(rec_d, (n,), vs.GUIDED_REC_DTYPE)
    eng.close()
    med = lambda v: round(float(np.median(v[1:])), 4)  # noqa: E731
    nbytes = n * ns * 6
    floor_ms = nbytes / (args.hbm_tbs * 1e12) * 1e3
    print(json.dumps({"what": "psola, " + label, "lanes": n, "samples": ns, "psola_ms": med(psola),
                      "psola_all_ms": [round(v, 4) for v in psola], "guided_ms": med(guided), "strack_ms": med(strack),
                      "bytes_gb": round(nbytes / 1e9, 3), "floor_ms_at_hbm_rate": round(floor_ms, 3),
                      "launch_share_of_hbm_rate": round(floor_ms / med(psola), 4),
                      "mean_marks": round(float(rec["n_marks"].mean()), 2), "mean_synth": round(float(st["n_synth"].mean()), 2),
                      "mean_governed": round(float(st["n_governed"].mean()), 2), "clipped": int(st["n_clipped"].sum()),
                      "rows_done": int((st["n_runs_done"] > 0).sum()), "status_or": int(np.bitwise_or.reduce(st["status"]))}))


if __name__ == "__main__":
    main()
