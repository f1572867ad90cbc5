#!/usr/bin/env python3
"""Device time of the coefficient-track filter (vs_track_launch) on config 3's flows (65536 x 16000 int16, 2.1 GB),
already on the device: Plan.launch(VS_KIND_SOURCE) writes them, every case below filters them on the same stream.

Per order (22: the tables' class; 40: the wide class, random stable sets):
    (a) the filter-only path the library already had: Plan.launch(VS_KIND_FILTER) (order 22: the fused kernels'
        filter-only kind; order 40: vs_filter_wide_kernel), one set per row;
    (b) hold, K = 1;  (c) hold, 100 sets per row (hop 160);
    (d) glide, 11 anchors (hop 1600) and 100 anchors (hop 160).
Every case: --warm launches, then --reps launches timed one by one with the vs_ctx timer events (median and minimum),
then --reps launches back to back between one pair of events (per launch).  One JSON line per case with the op-count
bound next to it: fp64 instructions (one per tap and sample with fused multiply-adds, two without; the step-up's
p(p-1)/2 multiply-adds per 24 samples in glide mode) at the 39.3e12 fp64 vector instructions per second of the chip.
Under `rocprofv3 --kernel-trace --stats -- python tools/track_bench.py` the kernels appear as vs_track_kernel<...>.

    python tools/track_bench.py [--lanes 65536] [--warm 10] [--reps 20] [--orders 22,40] [--arith exact|fma]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voice_synth_amd as vs  # noqa: E402
from voice_synth_amd import configs  # noqa: E402

FP64_INSTR_PER_S = 39.3e12   # 78.6 TF fp64 vector peak, an FMA counted as two


def step_up(kappa):
    """A[..., 0..p] of reflection coefficients kappa[..., p] (the header's step-up)"""
    p = kappa.shape[-1]
    a = np.zeros(kappa.shape[:-1] + (p + 1,))
    a[..., 0] = 1.0
    t = a[..., 1:]
    for i in range(1, p + 1):
        ki = kappa[..., i - 1]
        if i > 1:
            t[..., :i - 1] = t[..., :i - 1] + ki[..., None] * t[..., i - 2::-1]
        t[..., i - 1] = ki
    return a


def set_pool(order, rng, size=4096):
    """stable sets: convex blends of the tables in the reflection domain, small further coefficients beyond 22 taps"""
    kt = np.array([vs.track_reflection(vs.vowel_coefficients(v)) for v in "aiu1234567"])
    a, b = rng.integers(0, 10, size), rng.integers(0, 10, size)
    w = rng.uniform(0, 1, (size, 1))
    k = w * kt[a] + (1.0 - w) * kt[b]
    k = k[:, :order] if order <= 22 else np.concatenate([k, rng.uniform(-0.2, 0.2, (size, order - 22))], axis=1)
    return step_up(k)


def timed(eng, launch, warm, reps):
    for _ in range(warm):
        launch()
    one = []
    for _ in range(reps):
        eng.timer_mark(0)
        launch()
        eng.timer_mark(1)
        one.append(eng.timer_elapsed())
    eng.timer_mark(0)
    for _ in range(reps):
        launch()
    eng.timer_mark(1)
    return float(np.median(one)), float(np.min(one)), eng.timer_elapsed() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--orders", default="22,40")
    ap.add_argument("--arith", default="exact", choices=("exact", "fma"))
    args = ap.parse_args()
    n = args.lanes
    eng = vs.Engine(0, arith=vs.VS_ARITH_EXACT if args.arith == "exact" else vs.VS_ARITH_FMA)
    specs, fs, dur, label = configs.config_specs(3, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    plan = eng.plan(lanes, ns)
    flow_d, out_d = eng.dev_alloc(n * pitch * 2), eng.dev_alloc(n * pitch * 2)
    st_d = eng.dev_alloc(n * 8)
    plan.launch(vs.VS_KIND_SOURCE, flow_d, pitch)
    assert plan.status() == 0
    rng = np.random.default_rng(3)
    per_tap = 2 if args.arith == "exact" else 1

    def report(what, order, K, mode, t, stepups):
        instr = n * ns * order * per_tap + n * (ns / 24.0) * stepups * order * (order - 1)
        med, lo, b2b = t
        print(json.dumps({"what": what, "order": order, "sets": K, "mode": mode, "arith": args.arith, "lanes": n,
                          "median_ms": round(med, 4), "min_ms": round(lo, 4), "back_to_back_ms": round(b2b, 4),
                          "bound_ms": round(instr / FP64_INSTR_PER_S * 1e3, 4),
                          "x_bound": round(b2b / (instr / FP64_INSTR_PER_S * 1e3), 2)}), flush=True)

    for order in [int(o) for o in args.orders.split(",")]:
        pool = set_pool(order, rng)
        # (a) the filter-only plan path with one set per row
        if order == 22:
            fplan, what = plan, "(a) Plan.launch(VS_KIND_FILTER), the tables of config 3"
        else:
            protos = [vs.set_coefficients(vs.default_lane(), pool[i]) for i in range(64)]
            arr = (vs.Lane * n)()
            for i in range(n):
                C.memmove(C.byref(arr[i]), C.byref(protos[i % 64]), C.sizeof(vs.Lane))
            fplan, what = eng.plan(arr, ns), "(a) Plan.launch(VS_KIND_FILTER), wide kernel"
        t = timed(eng, lambda: fplan.launch(vs.VS_KIND_FILTER, out_d, pitch, flow_d, pitch), args.warm, args.reps)
        assert fplan.status() == 0
        report(what + " [%s]" % fplan.kernel_name(vs.VS_KIND_FILTER), order, 1, "plan", t, 0)
        if fplan is not plan:
            fplan.close()
        for mode, K, hop in (("hold", 1, 160), ("hold", 100, 160), ("glide", 11, 1600), ("glide", 100, 160)):
            coefs = pool[rng.integers(0, len(pool), (n, K))]
            cf_d = eng.dev_alloc(coefs.nbytes)
            eng.dev_upload(cf_d, coefs)
            del coefs
            rows = vs.track_rows(n, K, hop, 0, ns, 1.0, 1.0)
            t = timed(eng, lambda: eng.filter_track_dev(mode, order, flow_d, pitch, out_d, pitch, n, ns, rows, cf_d, K,
                                                        stat_ptr=st_d), args.warm, args.reps)
            st = eng.dev_download(st_d, (n,), vs.TRACK_STAT_DTYPE)
            assert not st["status"].any() and not st["n_unusable"].any()
            eng.dev_free(cf_d)
            report("(%s) vs_track_launch" % ("b" if K == 1 else "c" if mode == "hold" else "d"), order, K, mode, t,
                   1 if mode == "glide" else 0)
    plan.close()
    for p in (flow_d, out_d, st_d):
        eng.dev_free(p)
    eng.close()


if __name__ == "__main__":
    main()
