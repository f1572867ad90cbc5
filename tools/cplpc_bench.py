#!/usr/bin/env python3
"""Device time of the closed-phase covariance LPC (vs_cplpc_launch) next to vs_lpc_launch and vs_iaif_launch of the same
batch, in the same run on the same buffers: config 3's vowels (65536 x 16000 int16, 2.1 GB) are written on the device by
Plan.launch(VS_KIND_SYNTH); the first pass (vs_iaif_launch -> vs_inverse_launch -> vs_measure_launch ->
vs_glottal_launch) runs once and leaves the cycle records on the device; then each of the three analyses is timed on its
own on the context's stream, at order 22, coefficients written, no formants.

Every case: --warm launches, then --reps launches timed one by one with the vs_ctx timer events (median and minimum),
then --reps launches back to back between one pair of events (per launch).  One JSON line per case.  For vs_cplpc_launch
the line carries the bytes the definition needs -- 2 per sample of every pooled span, 48 per cycle record read, the
56-byte and 32-byte records read and the 32 + 8 * (order + 1) + 8 bytes written per row -- the time those bytes take at
the 8.0 TB/s of the chip's HBM3E (bound_ms) and the share of that roofline reached.  A second run with min_equations
2^31 - 1 refuses every frame before the solve: what is left is the covariance stage alone, and the difference is the
solve, the step-down and the records: the last line says which of the two binds.

    python tools/cplpc_bench.py [--config 3] [--lanes 65536] [--warm 3] [--reps 5] [--out profiles/cplpc_config3.txt]

--config 2 --lanes 65536 is the same number of rows without glottal noise: every cycle has a closed phase to pool.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voice_synth_amd as vs  # noqa: E402
from voice_synth_amd import configs  # noqa: E402
from track_bench import timed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12        # HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", type=int, default=22)
    ap.add_argument("--config", type=int, default=3, help="the batch: 3 (glottal noise: few closures), 2 (clean /a/) ...")
    ap.add_argument("--cycles", type=int, default=200, help="marks_pitch and cycles_pitch (config 3 has at most 137 marks)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    n, cp, p = args.lanes, args.cycles, args.order
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(args.config, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    A, G, Cy, F = vs.ACOUSTIC_DTYPE, vs.GLOTTAL_DTYPE, vs.GLOTTAL_CYCLE_DTYPE, vs.LPC_FRAME_DTYPE
    ikw = dict(order=p, n_formants=0)
    ilo = vs.iaif_lpc_opts(**ikw)
    fp = vs.lpc_frames(fs, ns, **ilo)
    row1 = vs.inverse_from_lpc(fs, ns, "hold", **ilo)
    row1["scale"], row1["de_emphasis"] = 0.1, 0.99
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d, res_d = dev.room(n * pitch * 2), dev.room(n * pitch * 2)
        fr_d, cf_d = dev.room(n * fp * F.itemsize), dev.room(n * fp * (p + 1) * 8)
        meas_d, marks_d, gl_d, cyc_d = dev.room(n * A.itemsize), dev.room(n * cp * 4), dev.room(n * G.itemsize), dev.room(n * cp * Cy.itemsize)
        cfr_d, ccf_d, cnt_d = dev.room(n * F.itemsize), dev.room(n * (p + 1) * 8), dev.room(n * 8)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        assert plan.status() == 0
        name, cus = eng.device_info()
        emit({"what": "cplpc_bench", "device": name.strip(), "cus": cus, "config": label, "lanes": n, "samples": ns,
              "order": p, "frames_per_row": fp, "cycles_pitch": cp, "warm": args.warm, "reps": args.reps})

        tl = timed(eng, lambda: eng.lpc_dev(pcm_d, pitch, n, ns, fs, fp, fr_d, None, cf_d, order=p, n_formants=0),
                   args.warm, args.reps)
        emit({"what": "vs_lpc_launch", "median_ms": round(tl[0], 4), "min_ms": round(tl[1], 4), "back_to_back_ms": round(tl[2], 4)})
        ti = timed(eng, lambda: eng.iaif_dev(pcm_d, pitch, n, ns, fs, fp, fr_d, None, cf_d, None, **ikw), args.warm, args.reps)
        emit({"what": "vs_iaif_launch", "median_ms": round(ti[0], 4), "min_ms": round(ti[1], 4), "back_to_back_ms": round(ti[2], 4)})
        # the first pass: IAIF's sets are in cf_d
        eng.inverse_filter_dev("hold", p, pcm_d, pitch, res_d, pitch, n, ns, row1, cf_d, fp)
        eng.measure_dev(res_d, pitch, n, ns, fs, meas_d, marks_ptr=marks_d, marks_pitch=cp)
        eng.glottal_dev(res_d, pitch, n, ns, meas_d, marks_d, cp, gl_d, cycles_ptr=cyc_d, cycles_pitch=cp)
        eng.synchronize()
        rec = dev.get(gl_d, (n,), G)
        assert (rec["n_cycles"] + rec["n_rejected"]).max() <= cp

        def run(**kw):
            return timed(eng, lambda: eng.cplpc_dev(pcm_d, pitch, n, ns, fs, gl_d, cyc_d, cp, 1, cfr_d, None, ccf_d, cnt_d,
                                                    order=p, n_formants=0, **kw), args.warm, args.reps)

        tc = run()
        eng.synchronize()
        fr, cnt = dev.get(cfr_d, (n,), F), dev.get(cnt_d, (n, 2), np.int32)
        nbytes = int((cnt[:, 1] + p * cnt[:, 0]).sum()) * 2 + int((rec["n_cycles"] + rec["n_rejected"]).sum()) * Cy.itemsize \
            + n * (G.itemsize + 32 + F.itemsize + 8 * (p + 1) + 8)
        bound = nbytes / HBM_BYTES_PER_S * 1e3
        with np.errstate(all="ignore"):
            q = fr["err"] / fr["r0"]
        emit({"what": "vs_cplpc_launch", "median_ms": round(tc[0], 4), "min_ms": round(tc[1], 4),
              "back_to_back_ms": round(tc[2], 4), "bytes": nbytes, "bound_ms": round(bound, 4),
              "hbm_fraction": round(bound / tc[2], 4), "rows_status_0": int((fr["status"] == 0).sum()),
              "spans": int(cnt[:, 0].sum()), "equations": int(cnt[:, 1].sum()),
              "median_err_over_r0": float(np.nanmedian(q))})
        t0 = run(min_equations=2 ** 31 - 1)
        emit({"what": "vs_cplpc_launch, every frame refused before the solve (covariance stage alone)",
              "median_ms": round(t0[0], 4), "min_ms": round(t0[1], 4), "back_to_back_ms": round(t0[2], 4)})
        solve = tc[2] - t0[2]
        emit({"what": "stages", "covariance_ms": round(t0[2], 4), "solve_and_records_ms": round(solve, 4),
              "binding_stage": "covariance" if t0[2] > solve else "solve",
              "cplpc / lpc": round(tc[2] / tl[2], 3), "cplpc / iaif": round(tc[2] / ti[2], 3)})
    eng.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
