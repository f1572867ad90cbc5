#!/usr/bin/env python3
"""The figures of README, "guided marks": what the guided walk does on the pitch track's constructed signals and on the
16 oracle vowels of the `vclosed` section, from the numpy restatements of tests/ alone (no device).

    python tools/guided_table.py            # every row
    python tools/guided_table.py signals    # the constructed signals only

The vowels' set-up is tools/cplpc_table.py's, with one change: the first pass's marks come from guided_ref (the residual's
pitch track, VS_MG_LONGEST) at the DEFAULT pitch range.  "read guided" reads a signal's shimmer, OQ, QOQ and NAQ through
guided marks, "read default" through acoustic_ref's.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import voice_synth_amd as vs  # noqa: E402

import acoustic_ref as ar  # noqa: E402
import guided_ref as gr  # noqa: E402
import pitch_signals as ps  # noqa: E402

FS = 22050


def signals():
    x, peaks, _ = ps.glide()
    for name, sig, kw in (("glide", x, {}), ("gaps", ps.gaps(), {}), ("gaps, edge_frames 0", ps.gaps(), dict(edge_frames=0)),
                          ("octave trap", ps.octave_trap(), {})):
        out, mk, rec, sg, _ = gr.track_and_guided(sig[None], 16000, marks=400, segs=8, **kw)
        m = mk[0][:rec["n_marks"][0]]
        T = np.concatenate([np.diff(m[s["first_mark_index"]:s["first_mark_index"] + s["n_marks"]])
                            for s in sg[0][:rec["n_segments"][0]]])
        plain = ar.measure(sig[None], 16000)[0]
        print("%-20s segments %d (frames %s), marks %s, K %d, periods %d..%d, jitter_local %.5f, shimmer_local %.5f, status %d"
              % (name, rec["n_segments"][0], "+".join(str(s["n_frames"]) for s in sg[0][:rec["n_segments"][0]]),
                 "+".join(str(s["n_marks"]) for s in sg[0][:rec["n_segments"][0]]), out["n_periods"][0], T.min(), T.max(),
                 out["jitter_local"][0], out["shimmer_local"][0], out["status"][0]))
        print("%-20s vs_measure: P0 %d, K %d, jitter_local %.5f, status %d" % ("", plain["p0"], plain["n_periods"],
                                                                             plain["jitter_local"], plain["status"]))
        if name == "glide":
            pk = np.asarray(peaks)
            print("%-20s peaks %d, marked within 1 sample: %d" % ("", len(pk), sum(np.abs(m - p).min() <= 1 for p in pk)))


def read(x, guided):
    import cplpc_table
    if not guided:
        r = cplpc_table.read(x)
        r["periods"] = ar.measure(x, FS)["n_periods"]
        return r
    meas, _, rec, _ = gr.measure_and_glottal(x, FS)
    out = {"shimmer": float(np.nanmean(meas["shimmer_local"])), "periods": meas["n_periods"]}
    for q in ("oq", "qoq", "naq"):
        out[q] = float(np.nanmean(rec[q]))
    return out


def vowels(flowgen_args, n=16):
    from oracle import pyoracle
    specs = [(["-d", "1", "-f", "100"] + list(flowgen_args), ["-v", "a"], 300 + k) for k in range(n)]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(FS, d)
    pcm, flow = pyoracle.synth(lanes, ns), pyoracle.source(lanes, ns)
    got = gr.closed_phase(pcm, FS, de_emphasis=1.0, scale=1.0 / lanes[0].gain)
    s = got["sets"]
    with np.errstate(all="ignore"):
        q = s["err"][:, 0] / s["r0"][:, 0]
    st = s["status"][:, 0]
    T = [float(np.diff(m[m >= 0]).mean()) if (m >= 0).sum() > 1 else float("nan") for m in got["marks"]]
    label = "`%s`" % " ".join(flowgen_args)
    print("%s: guided first pass: K %d..%d, mean period %.1f..%.1f; sets: status 0 in %d of %d (statuses %s), err / r0 %.1e .. %.1e"
          % (label, got["meas"]["n_periods"].min(), got["meas"]["n_periods"].max(), np.nanmin(T), np.nanmax(T),
             (st == 0).sum(), n, sorted(set(st.tolist())), np.nanmin(q), np.nanmax(q)))
    for name, x, g in (("flow, read default", flow, False), ("flow, read guided", flow, True),
                       ("closed-phase flow, read default", got["flow"], False),
                       ("closed-phase flow, read guided", got["flow"], True)):
        r = read(x, g)
        print("| %-12s | %-32s | %.4f | %.5f | %.5f | %.4f | K %d..%d |" % (label, name, r["shimmer"], r["oq"], r["qoq"], r["naq"],
                                                                        r["periods"].min(), r["periods"].max()))


if __name__ == "__main__":
    signals()
    if sys.argv[1:] != ["signals"]:
        for args in (("-s", "10"), ("-s", "2"), ("-s", "5", "-j", "2"), ("-s", "2", "-n", "20")):
            vowels(args)
