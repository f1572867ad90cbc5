#!/usr/bin/env python3
"""Device time of ONE IAIF analysis (vs_iaif_launch) and of ONE LPC analysis (vs_lpc_launch) of config 3's batch
(65536 x 16000 int16, 2.1 GB), already on the device, in the same run on the same box: synthesised there by
Plan.launch(VS_KIND_SYNTH), then analysed on the same stream.  Order 22, glottal order 4, 25 ms Hamming window, 10 ms
hop (98 frames per row, 6.4 M frames), with 0 and with 5 formants.  The vs_ctx timer events bracket each analysis alone;
one JSON line per (formants, analysis): the median of --reps after one warm-up, with the op-count bound of the analysis
at the 78.6 TF fp64 vector peak, and IAIF's ratio to vs_lpc.  Under `rocprofv3 --kernel-trace --stats -- python
tools/iaif_bench.py` the kernels appear as vs_iaif_kernel and vs_lpc_kernel.

    python tools/iaif_bench.py [--lanes 65536] [--reps 5] [--order 22] [--glottal 4]
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
    ap.add_argument("--glottal", type=int, default=4)
    args = ap.parse_args()
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, args.lanes)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    n, p, g = args.lanes, args.order, args.glottal
    plan = eng.plan(lanes, ns)
    pcm_d = eng.dev_alloc(n * pitch * 2)
    plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
    nfr = vs.lpc_frames(fs, ns, order=p)
    L = int(np.floor(0.025 * fs + 0.5))
    fr_d = eng.dev_alloc(n * nfr * vs.LPC_FRAME_DTYPE.itemsize)
    fm_d = eng.dev_alloc(n * nfr * 10 * 8)
    # multiply-adds per frame: the autocorrelations of the four stages and their FIRs; vs_lpc: one autocorrelation
    fma = {"iaif": L * (2 + (p + 1) + (g + 1) + (p + 1)) + L * (1 + p + g), "lpc": L * (p + 1)}
    for formants in (0, 5):
        ms = {}
        for what in ("lpc", "iaif"):
            times = []
            for _ in range(args.reps + 1):
                eng.timer_mark(0)
                if what == "lpc":
                    eng.lpc_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, fm_d, order=p, n_formants=formants)
                else:
                    eng.iaif_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, fm_d, order=p, glottal_order=g, n_formants=formants)
                eng.timer_mark(1)
                times.append(eng.timer_elapsed())
            fr = eng.dev_download(fr_d, (n, nfr), vs.LPC_FRAME_DTYPE)
            ms[what] = float(np.median(times[1:]))
            macs = n * nfr * fma[what]
            print(json.dumps({"what": "%s analysis, track, %s" % (what.upper(), label), "lanes": n, "frames": n * nfr,
                              "order": p, "glottal_order": g if what == "iaif" else None, "formants": formants,
                              "ms": round(ms[what], 4), "all_ms": [round(t, 4) for t in times], "multiply_adds": macs,
                              "fp64_bound_ms": round(2 * macs / 78.6e12 * 1e3, 4),
                              "ok_frames": int((fr["status"] == 0).sum()),
                              "no_roots": int((fr["status"] == vs.VS_LPC_NO_ROOTS).sum())}))
        print(json.dumps({"what": "IAIF / LPC", "formants": formants, "ratio": round(ms["iaif"] / ms["lpc"], 3),
                          "op_count_ratio": round(fma["iaif"] / fma["lpc"], 3)}))
    plan.close()
    for ptr in (pcm_d, fr_d, fm_d):
        eng.dev_free(ptr)
    eng.close()


if __name__ == "__main__":
    main()
