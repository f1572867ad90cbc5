#!/usr/bin/env python3
"""Device time of ONE launch of PSOLA with a time map (vs_psola_ts_launch: its plan kernel and its overlap-add kernel)
beside ONE vs_psola_launch, in one run, on config 3's batch (65536 x 16000 int16 at 16 kHz) already on the device: the
marks and the target of tools/psola_bench.py (one vs_guided_launch behind one vs_pitch_launch; the cycle log of one
vs_strack_launch on a vibrato track, read in place at strides 32 / 24).  Three launches are timed, each between the vs_ctx
timer events alone: vs_psola_launch; vs_psola_ts_launch with the identity map (the same samples, plus the unvoiced marks in
front of and behind every run); vs_psola_ts_launch with the output 1.5 times as long, whose target is the cycle log of a
second vs_strack_launch over the output's length on the same track held 1.5 times as long.  One JSON line (medians of
--reps) with the time the 6 bytes an OUTPUT sample (two int16 reads, one store) take at the HBM rate given.  The split
between the kernels comes from `rocprofv3 --kernel-trace --stats -- python tools/psola_ts_bench.py`, where they appear as
vs_pt_plan_kernel and vs_pt_ola_kernel beside vs_ps_plan_kernel and vs_ps_ola_kernel.

    python tools/psola_ts_bench.py [--lanes 65536] [--reps 5] [--hbm-tbs 8.0]
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
    no = ns * 3 // 2
    pitch, opitch = vs.row_pitch(ns), vs.row_pitch(no)
    n = args.lanes
    gp = vs.guided_plan(fs, ns)
    fp = max(1, gp["n_frames"])
    mp, sgp, cp, sp = 256, 4, 256, 512
    hop = int(math.floor(0.010 * fs + 0.5))
    tfp = -(-ns // hop)
    f0 = np.array([l.F0 for l in lanes], dtype=np.float64)
    t = (np.arange(tfp) * hop + hop // 2) / float(fs)
    vib = (float(fs) / (f0[:, None] * (1.0 + 0.05 * np.sin(2.0 * np.pi * 5.0 * t)[None, :]))).astype(np.int32)
    rows = vs.strack_rows(n, tfp, hop, 0, ns, gp["tmin"], gp["tmax"])
    orows = vs.strack_rows(n, tfp, hop * 3 // 2, 0, no, gp["tmin"], gp["tmax"])
    same, w = vs.psola_two_anchors([ns] * n, [ns] * n)
    longer, _ = vs.psola_two_anchors([ns] * n, [no] * n)
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        out_d = dev.room(n * opitch * 2)
        flow_d = dev.room(n * opitch * 2)
        fr_d = dev.room(n * fp * vs.PITCH_FRAME_DTYPE.itemsize)
        meas_d = dev.room(n * vs.ACOUSTIC_DTYPE.itemsize)
        rec_d = dev.room(n * vs.GUIDED_REC_DTYPE.itemsize)
        mk_d = dev.room(n * mp * 4)
        sg_d = dev.room(n * sgp * vs.GUIDED_SEG_DTYPE.itemsize)
        per_d = dev.put(vib)
        sst_d, osst_d = (dev.room(n * vs.STRACK_STAT_DTYPE.itemsize) for _ in range(2))
        cyc_d, ocyc_d = (dev.room(n * cp * vs.STRACK_CYCLE_DTYPE.itemsize) for _ in range(2))
        stat_d = dev.room(n * vs.PSOLA_STAT_DTYPE.itemsize)
        sy_d = dev.room(n * sp * vs.PSOLA_MARK_DTYPE.itemsize)
        same_d, longer_d, w_d = dev.put(same), dev.put(longer), dev.put(w)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        eng.pitch_dev(pcm_d, pitch, n, ns, fs, fp, fr_d)
        eng.measure_guided_dev(pcm_d, pitch, n, ns, fs, fr_d, fp, meas_d, rec_d, mk_d, mp, sg_d, sgp)
        eng.source_track_dev(lanes, ns, rows, per_d, 4, tfp, flow_d, pitch, sst_d, cycles_ptr=cyc_d, cycles_pitch=cp)
        eng.source_track_dev(lanes, no, orows, per_d, 4, tfp, flow_d, opitch, osst_d, cycles_ptr=ocyc_d, cycles_pitch=cp)
        kw = dict(segs_ptr=sg_d, seg_pitch=sgp, pmin=gp["tmin"], pmax=gp["tmax"])
        times = {"psola": [], "ts_identity": [], "ts_x1.5": []}
        stats = {}
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            eng.psola_dev(pcm_d, pitch, n, ns, mk_d, mp, rec_d, cyc_d, 32, cyc_d + 4, 32, sst_d + 4, 24, cp, out_d, pitch,
                          stat_d, sy_d, sp, **kw)
            eng.timer_mark(1)
            times["psola"].append(eng.timer_elapsed())
            stats["psola"] = dev.get(stat_d, (n,), vs.PSOLA_STAT_DTYPE)
            eng.timer_mark(0)
            eng.psola_ts_dev(pcm_d, pitch, n, ns, mk_d, mp, rec_d, cyc_d, 32, cyc_d + 4, 32, sst_d + 4, 24, cp, same_d, w_d, 2,
                             out_d, pitch, ns, stat_d, sy_d, sp, **kw)
            eng.timer_mark(1)
            times["ts_identity"].append(eng.timer_elapsed())
            stats["ts_identity"] = dev.get(stat_d, (n,), vs.PSOLA_STAT_DTYPE)
            eng.timer_mark(0)
            eng.psola_ts_dev(pcm_d, pitch, n, ns, mk_d, mp, rec_d, ocyc_d, 32, ocyc_d + 4, 32, osst_d + 4, 24, cp, longer_d,
                             w_d, 2, out_d, opitch, no, stat_d, sy_d, sp, **kw)
            eng.timer_mark(1)
            times["ts_x1.5"].append(eng.timer_elapsed())
            stats["ts_x1.5"] = dev.get(stat_d, (n,), vs.PSOLA_STAT_DTYPE)
    eng.close()
    med = lambda v: round(float(np.median(v[1:])), 4)  # noqa: E731
    out = {"what": "psola with a time map, " + label, "lanes": n, "samples": ns, "samples_x1.5": no}
    for key, length in (("psola", ns), ("ts_identity", ns), ("ts_x1.5", no)):
        st = stats[key]
        floor_ms = n * length * 6 / (args.hbm_tbs * 1e12) * 1e3
        out[key] = {"ms": med(times[key]), "all_ms": [round(v, 4) for v in times[key]],
                    "floor_ms_at_hbm_rate": round(floor_ms, 3), "launch_share_of_hbm_rate": round(floor_ms / med(times[key]), 4),
                    "mean_synth": round(float(st["n_synth"].mean()), 2), "mean_governed": round(float(st["n_governed"].mean()), 2),
                    "clipped": int(st["n_clipped"].sum()), "status_or": int(np.bitwise_or.reduce(st["status"]))}
    out["ts_identity_over_psola"] = round(out["ts_identity"]["ms"] / out["psola"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
