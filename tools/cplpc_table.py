#!/usr/bin/env python3
"""The table of README, "vclosed": what the glottal measurements read on the flow the closed-phase sets recover, beside
the flow itself and beside IAIF's sets, from the numpy restatements of tests/ alone (no device).

    python tools/cplpc_table.py            # the README's rows
    python tools/cplpc_table.py -s 7 -j 1  # one row with these flowgen_shimmer arguments

Set-up (tests/test_cplpc_ref.py asserts the first three rows): 16 oracle vowels `-v a`, gain 10, pre-emphasis 1, F0 100,
22050 Hz, 1 s, seeds 300..315, order 22.  First pass: IAIF sets at their defaults, inverse in hold mode with de-emphasis
0.99 and scale 1/10, acoustic_ref.measure, glottal_ref at levels 26 / 128.  Closed-phase estimate at its defaults (spans
[close + 4, close + 4 + 0.3 period), one set per row).  Second pass: inverse with that set -- and, for comparison, with
IAIF's sets -- at de-emphasis 1 and scale 1/10.  Every signal is then measured the same way: mean over the rows of the
local shimmer (acoustic_ref) and of OQ, QOQ and NAQ (glottal_ref, levels 26 / 128), at the default pitch range.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voice_synth_amd as vs  # noqa: E402
from oracle import pyoracle  # noqa: E402

import acoustic_ref as ar  # noqa: E402
import cplpc_ref as cp  # noqa: E402
import glottal_ref as gl  # noqa: E402
import inverse_ref as ir  # noqa: E402
import lpc_ref as lr  # noqa: E402

FS = 22050
QUANTITIES = ("shimmer", "oq", "qoq", "naq")


def read(x, level_open=26):
    """the four means of the rows of x"""
    meas, _, rec = gl.measure_and_glottal(x, FS, level_open, 128)
    out = {"shimmer": float(np.nanmean(meas["shimmer_local"]))}
    for q in ("oq", "qoq", "naq"):
        out[q] = float(np.nanmean(rec[q]))
    return out


@functools.lru_cache(maxsize=None)
def table(flowgen_args, f0_min=50.0, n=16, level_open=26):
    """one row of the table for flowgen_shimmer arguments (a tuple of str): dict flow / iaif / closed (each read()'s
    dict), status and err_over_r0 [rows] of the closed-phase sets, tap_error [rows] = max |a_j - table|, periods"""
    specs = [(["-d", "1", "-f", "100"] + list(flowgen_args), ["-v", "a"], 300 + k) for k in range(n)]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(FS, d)
    pcm = pyoracle.synth(lanes, ns)
    flow = pyoracle.source(lanes, ns)
    scale = 1.0 / lanes[0].gain
    got = cp.closed_phase(pcm, FS, de_emphasis=1.0, scale=scale, f0_min=f0_min, level_open=level_open)
    iaif = got["iaif"]
    L, H, starts = lr.frame_plan(FS, ns, lr.opts())
    n_sets, hop, offset, _ = ir.from_lpc(L, H, 0, len(starts), ns, ir.HOLD)[:4]
    rows = ir.rows_of(n, n_sets, hop, offset, ns, scale, 1.0)
    by_iaif = ir.inverse_filter(pcm, iaif["coefs"], rows, ir.HOLD)[0]
    s = got["sets"]
    A = vs.vowel_coefficients("a")
    with np.errstate(all="ignore"):
        q = s["err"][:, 0] / s["r0"][:, 0]
    return dict(flow=read(flow, level_open), iaif=read(by_iaif, level_open), closed=read(got["flow"], level_open),
                status=s["status"][:, 0].copy(), err_over_r0=q, tap_error=np.abs(s["coefs"][:, 0] - A[None, :]).max(axis=1),
                periods=got["meas"]["p0"].copy(), counts=s["counts"][:, 0].copy())


def show(label, t):
    for name, key in (("flow", "flow"), ("IAIF sets (de-emphasis 1)", "iaif"), ("closed-phase sets", "closed")):
        print("| %-28s | %-26s | %.4f | %.4f | %.4f | %.4f |" % ((label if key == "flow" else "", name)
                                                                 + tuple(t[key][q] for q in QUANTITIES)))
    ok = t["status"] == 0
    print("    status 0 in %d of %d rows; err / r0 %.1e .. %.1e; max |a_j - table| %.3f .. %.3f; first-pass periods %d .. %d"
          % (ok.sum(), len(ok), np.nanmin(t["err_over_r0"]), np.nanmax(t["err_over_r0"]), np.nanmin(t["tap_error"]),
             np.nanmax(t["tap_error"]), t["periods"].min(), t["periods"].max()))


ROWS = ((("-s", "2"), 50.0, 26), (("-s", "5", "-j", "2"), 50.0, 26), (("-s", "10"), 70.0, 26), (("-s", "10"), 50.0, 26),
        (("-s", "2", "-n", "20"), 50.0, 26), (("-s", "2", "-n", "20"), 50.0, 51))

if __name__ == "__main__":
    print("| flowgen args | signal | shimmer | OQ | QOQ | NAQ |")
    print("|---|---|---|---|---|---|")
    if len(sys.argv) > 1:
        show(" ".join(sys.argv[1:]), table(tuple(sys.argv[1:])))
    else:
        for args, f0_min, level in ROWS:
            label = "`%s`" % " ".join(args) + (", first-pass f0_min %g" % f0_min if f0_min != 50.0 else "") \
                + (", level_open %d" % level if level != 26 else "")
            show(label, table(args, f0_min, 16, level))
