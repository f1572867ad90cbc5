#!/usr/bin/env python3
"""Device time of the inverse filter (vs_inverse_launch) next to the coefficient-track filter (vs_track_launch) of the
same shape, in the same run on the same box: config 3's flows (65536 x 16000 int16, 2.1 GB) are written on the device by
Plan.launch(VS_KIND_SOURCE) and filtered once by vs_track (hold, K = 1, table 'a', gain 0.25) into the speech; every case
below then runs on that speech (inverse) or on the flows (track) on the same stream.

Per order (22: the tables' class; 40: the wide class, random stable sets) and arithmetic (exact, fma):
    hold, K = 1;  hold, 100 sets per row (hop 160);  glide, 11 anchors (hop 1600) and 100 anchors (hop 160).
Every case: --warm launches, then --reps launches timed one by one with the vs_ctx timer events (median and minimum),
then --reps launches back to back between one pair of events (per launch).  One JSON line per case with the op-count
bound next to it: fp64 instructions per sample (one per tap with fused multiply-adds, two without; the recurrence of u
the same; one for the scale; in glide mode the step-up's p(p-1)/2 multiply-adds per 24 samples) at the 39.3e12 fp64
vector instructions per second of the chip.  The track filter has the same multiply-adds in one dependent chain per
sample; the inverse has them without that chain.

    python tools/inverse_bench.py [--lanes 65536] [--warm 5] [--reps 10] [--orders 22,40] [--out profiles/inverse_config3.txt]
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
from track_bench import FP64_INSTR_PER_S, set_pool, timed  # noqa: E402

SHAPES = (("hold", 1, 160), ("hold", 100, 160), ("glide", 11, 1600), ("glide", 100, 160))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--orders", default="22,40")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    n = args.lanes
    eng = vs.Engine(0)
    specs, fs, dur, label = configs.config_specs(3, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    plan = eng.plan(lanes, ns)
    flow_d, speech_d, out_d = (eng.dev_alloc(n * pitch * 2) for _ in range(3))
    tst_d, ist_d = eng.dev_alloc(n * 8), eng.dev_alloc(n * 16)
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
    emit({"what": "inverse_bench", "device": name.strip(), "cus": cus, "config": label, "lanes": n, "samples": ns,
          "warm": args.warm, "reps": args.reps})
    # the speech: the flows through table 'a', held
    A = np.ascontiguousarray(np.broadcast_to(vs.vowel_coefficients("a"), (n, 1, 23)))
    a_d = eng.dev_alloc(A.nbytes)
    eng.dev_upload(a_d, A)
    eng.filter_track_dev("hold", 22, flow_d, pitch, speech_d, pitch, n, ns, vs.track_rows(n, 1, 160, 0, ns, 0.25, 1.0), a_d,
                         1, stat_ptr=tst_d)
    eng.synchronize()
    eng.dev_free(a_d)
    del A
    rng = np.random.default_rng(3)

    def report(what, order, K, mode, arith, per_sample, t, stepups):
        instr = n * ns * per_sample + n * (ns / 24.0) * stepups * order * (order - 1)
        med, lo, b2b = t
        bound = instr / FP64_INSTR_PER_S * 1e3
        emit({"what": what, "order": order, "sets": K, "mode": mode, "arith": arith, "median_ms": round(med, 4),
              "min_ms": round(lo, 4), "back_to_back_ms": round(b2b, 4), "bound_ms": round(bound, 4),
              "x_bound": round(b2b / bound, 2)})
        return b2b

    for order in [int(o) for o in args.orders.split(",")]:
        pool = set_pool(order, rng)
        for mode, K, hop in SHAPES:
            coefs = pool[rng.integers(0, len(pool), (n, K))]
            cf_d = eng.dev_alloc(coefs.nbytes)
            eng.dev_upload(cf_d, coefs)
            del coefs
            trows = vs.track_rows(n, K, hop, 0, ns, 1.0, 1.0)
            irows = vs.inverse_rows(n, K, hop, 0, ns, 1.0, 1.0)
            glide = 1 if mode == "glide" else 0
            for arith in ("exact", "fma"):
                eng.set_arith(vs.VS_ARITH_EXACT if arith == "exact" else vs.VS_ARITH_FMA)
                per_tap = 2 if arith == "exact" else 1
                t = timed(eng, lambda: eng.filter_track_dev(mode, order, flow_d, pitch, out_d, pitch, n, ns, trows, cf_d, K,
                                                            stat_ptr=tst_d), args.warm, args.reps)
                st = eng.dev_download(tst_d, (n,), vs.TRACK_STAT_DTYPE)
                assert not st["status"].any() and not st["n_unusable"].any()
                # x*gain, the taps, the pre-emphasis
                tt = report("vs_track_launch", order, K, mode, arith, 1 + order * per_tap + per_tap, t, glide)
                t = timed(eng, lambda: eng.inverse_filter_dev(mode, order, speech_d, pitch, out_d, pitch, n, ns, irows, cf_d,
                                                              K, stat_ptr=ist_d), args.warm, args.reps)
                st = eng.dev_download(ist_d, (n,), vs.INVERSE_STAT_DTYPE)
                assert not st["status"].any() and not st["n_unusable"].any()
                # the de-emphasis, the taps, e*scale
                ti = report("vs_inverse_launch", order, K, mode, arith, per_tap + order * per_tap + 1, t, glide)
                emit({"what": "inverse / track", "order": order, "sets": K, "mode": mode, "arith": arith,
                      "ratio": round(ti / tt, 3), "clipped_share": round(float(st["n_clipped"].sum()) / (n * ns), 4)})
            eng.dev_free(cf_d)
    eng.set_arith(vs.VS_ARITH_EXACT)
    plan.close()
    for p in (flow_d, speech_d, out_d, tst_d, ist_d):
        eng.dev_free(p)
    eng.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
