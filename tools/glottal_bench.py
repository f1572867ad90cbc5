#!/usr/bin/env python3
"""Device time of the glottal parameters (vs_glottal_launch) next to the measurement it chains behind
(vs_measure_launch), in the same run on the same buffers: config 3's flows (65536 x 16000 int16, 2.1 GB) are written on
the device by Plan.launch(VS_KIND_SOURCE), measured once (records and marks stay on the device), and then each of the two
launches is timed on its own on the context's stream.

Every case: --warm launches, then --reps launches timed one by one with the vs_ctx timer events (median and minimum),
then --reps launches back to back between one pair of events (per launch).  One JSON line per case.  For vs_glottal_launch
the line carries the bytes the definition needs -- 2 per sample of every row with cycles, 4 per mark read, the 96-byte
record read and the 56-byte record written per row (no cycle records are asked for) -- the time those bytes take at the
8.0 TB/s of the chip's HBM3E (bound_ms) and the share of that roofline reached (hbm_fraction = bound_ms /
back_to_back_ms); the same share against the 6.29 TB/s a plain copy reaches is next to it.  The last line says whether
the pass costs less than the measurement in front of it.

    python tools/glottal_bench.py [--lanes 65536] [--warm 5] [--reps 10] [--out profiles/glottal_config3.txt]
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
COPY_BYTES_PER_S = 6.29e12      # what a float4 copy reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--marks", type=int, default=200, help="marks_pitch (config 3's flows have at most 137 marks)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    n, mp = args.lanes, args.marks
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    plan = eng.plan(lanes, ns)
    A, G = vs.ACOUSTIC_DTYPE, vs.GLOTTAL_DTYPE
    flow_d, meas_d, marks_d, out_d = (eng.dev_alloc(v) for v in (n * pitch * 2, n * A.itemsize, n * mp * 4, n * G.itemsize))
    plan.launch(vs.VS_KIND_SOURCE, flow_d, pitch)
    assert plan.status() == 0
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    name, cus = eng.device_info()
    emit({"what": "glottal_bench", "device": name.strip(), "cus": cus, "config": label + " (flows)", "lanes": n,
          "samples": ns, "marks_pitch": mp, "warm": args.warm, "reps": args.reps})

    tm = timed(eng, lambda: eng.measure_dev(flow_d, pitch, n, ns, fs, meas_d, marks_ptr=marks_d, marks_pitch=mp),
               args.warm, args.reps)
    eng.synchronize()
    meas = eng.dev_download(meas_d, (n,), A)
    assert meas["n_periods"].max() < mp
    emit({"what": "vs_measure_launch", "median_ms": round(tm[0], 4), "min_ms": round(tm[1], 4),
          "back_to_back_ms": round(tm[2], 4), "rows_measured": int((meas["status"] == 0).sum()),
          "periods": int(meas["n_periods"].sum())})

    for lo, mid in ((26, 128), (0, 128)):
        tg = timed(eng, lambda: eng.glottal_dev(flow_d, pitch, n, ns, meas_d, marks_d, mp, out_d, lo, mid), args.warm,
                   args.reps)
        eng.synchronize()
        rec = eng.dev_download(out_d, (n,), G)
        walked = (rec["n_cycles"] + rec["n_rejected"]) > 0
        nbytes = int(walked.sum()) * ns * 2 + int((meas["n_periods"][walked] + 1).sum()) * 4 + n * (A.itemsize + G.itemsize)
        bound = nbytes / HBM_BYTES_PER_S * 1e3
        emit({"what": "vs_glottal_launch", "level_open": lo, "level_mid": mid, "median_ms": round(tg[0], 4),
              "min_ms": round(tg[1], 4), "back_to_back_ms": round(tg[2], 4), "bytes": nbytes, "bound_ms": round(bound, 4),
              "hbm_fraction": round(bound / tg[2], 3), "of_copy_rate": round(nbytes / COPY_BYTES_PER_S * 1e3 / tg[2], 3),
              "cycles": int(rec["n_cycles"].sum()), "rejected": int(rec["n_rejected"].sum()),
              "mean_oq": round(float(np.nanmean(rec["oq"])), 4), "mean_naq": round(float(np.nanmean(rec["naq"])), 4)})
        if lo == 26:
            emit({"what": "glottal / measure", "ratio": round(tg[2] / tm[2], 3),
                  "glottal_costs_less_than_the_measurement": bool(tg[2] < tm[2])})
    plan.close()
    for p in (flow_d, meas_d, marks_d, out_d):
        eng.dev_free(p)
    eng.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
