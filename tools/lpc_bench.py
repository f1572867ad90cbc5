#!/usr/bin/env python3
"""Device time of ONE LPC analysis (vs_lpc_launch) of config 3's batch (65536 x 16000 int16, 2.1 GB), already on the
device: synthesised there by Plan.launch(VS_KIND_SYNTH), then analysed on the same stream.  Two modes: the 25 ms / 10 ms
track (98 frames per row, 6.4 M frames) and the centre frame (hop 0, one frame per row), both at order 22 with five
formants.  The vs_ctx timer events bracket the analysis alone; one JSON line per mode (median of --reps after one
warm-up), with the autocorrelation's exact multiply-adds and what they take at the 78.6 TF fp64 vector peak.  Under
`rocprofv3 --kernel-trace --stats -- python tools/lpc_bench.py` the kernel appears as vs_lpc_kernel.

    python tools/lpc_bench.py [--lanes 65536] [--reps 5] [--order 22] [--formants 5] [--mode track|centre|both]
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
    ap.add_argument("--order", type=int, default=22)
    ap.add_argument("--formants", type=int, default=5)
    ap.add_argument("--mode", default="both", choices=("track", "centre", "both"))
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n = args.lanes
    plan = eng.plan(lanes, ns)
    pcm_d = eng.dev_alloc(n * pitch * 2)
    eng.timer_mark(0)
    plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
    eng.timer_mark(1)
    synth_ms = eng.timer_elapsed()
    modes = ("track", "centre") if args.mode == "both" else (args.mode,)
    for mode in modes:
        kw = dict(order=args.order, n_formants=args.formants, hop_s=0.010 if mode == "track" else 0.0)
        nfr = vs.lpc_frames(fs, ns, **kw)
        fr_d = eng.dev_alloc(n * nfr * vs.LPC_FRAME_DTYPE.itemsize)
        fm_d = eng.dev_alloc(n * nfr * max(1, 2 * args.formants) * 8)
        times = []
        for _ in range(args.reps + 1):
            eng.timer_mark(0)
            eng.lpc_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, fm_d, **kw)
            eng.timer_mark(1)
            times.append(eng.timer_elapsed())
        fr = eng.dev_download(fr_d, (n, nfr), vs.LPC_FRAME_DTYPE)
        fm = eng.dev_download(fm_d, (n, nfr, args.formants, 2), np.float64) if args.formants else None
        eng.dev_free(fr_d)
        eng.dev_free(fm_d)
        ms = float(np.median(times[1:]))
        L = int(np.floor(0.025 * fs + 0.5))
        macs = n * nfr * L * (args.order + 1)  # upper bound: every lag over the whole window
        ok = fr["status"] == 0
        print(json.dumps({"what": "LPC analysis, %s, %s" % (mode, label), "lanes": n, "frames": n * nfr,
                          "order": args.order, "formants": args.formants, "lpc_ms": round(ms, 4),
                          "all_ms": [round(t, 4) for t in times], "synth_ms": round(synth_ms, 4),
                          "autocorr_macs": macs, "fp64_bound_ms": round(2 * macs / 78.6e12 * 1e3, 4),
                          "ok_frames": int(ok.sum()), "no_roots": int((fr["status"] == vs.VS_LPC_NO_ROOTS).sum()),
                          "mean_F1_Hz": float(np.nanmean(fm[..., 0, 0][ok])) if args.formants else None}))
    plan.close()
    eng.dev_free(pcm_d)
    eng.close()


if __name__ == "__main__":
    main()
