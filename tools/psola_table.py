#!/usr/bin/env python3
"""The figures of the README's PSOLA section, from the restatements alone (tests/psola_ref.py on the guided marks of
tests/guided_ref.py, the signals of tests/pitch_signals.py at 16 kHz): no GPU, no library.

    python tools/psola_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import guided_ref as gr  # noqa: E402
import pitch_signals as ps  # noqa: E402
import psola_ref as pp  # noqa: E402

FS = 16000


def guided(x):
    out, mk, rec, sg, _ = gr.track_and_guided(np.asarray(x)[None], FS, marks=400, segs=8)
    return out[0], mk, rec, sg


def psola(x, mk, rec, sg, start, T, gain=None, sp=800):
    start, T = np.asarray(start, dtype=np.int64)[None], np.asarray(T, dtype=np.int64)[None]
    y, st, sy = pp.psola(np.asarray(x)[None], [len(x)], mk, rec, sg, start, T, None if gain is None else np.asarray(gain)[None],
                         [start.shape[1]], 32, 320, sp)
    return y[0], st[0], sy[0]


def list_jitter(t):
    p = np.diff(np.asarray(t, dtype=np.float64))
    return float(np.abs(np.diff(p)).mean() / p.mean())


def constant(T, n=800):
    return np.arange(n) * T, [T] * n


def main():
    x, _ = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)
    out, mk, rec, sg = guided(x)
    print("train([123]*100): %d run, %d marks, jitter_local %.5f" % (rec["n_segments"][0], rec["n_marks"][0], out["jitter_local"]))
    for name, sig in (("glide()", ps.glide()[0]), ("gaps()", ps.gaps())):
        o, m, r, s = guided(sig)
        y, st, _ = psola(sig, m, r, s, [0], [0])
        print("identity, %s: %d runs, %d synthesis marks, y == x: %s" % (name, st["n_runs_done"], st["n_synth"], np.array_equal(y, sig)))
    rng = np.random.default_rng(3)
    T = rng.integers(119, 128, 140)
    start = np.cumsum(T) - T
    gains = rng.integers(int(0.85 * pp.Q), int(1.15 * pp.Q) + 1, 140)
    y, st, sy = psola(x, mk, rec, sg, start, T)
    t = sy["t"][:st["n_synth"]]
    o2, m2, r2, _ = guided(y)
    print("T uniform 119..127: %d synthesis marks, differences but the last equal T[0..98): %s; guided marks of y equal them: %s; "
          "jitter_local of y %.5f, of the list %.5f" % (st["n_synth"], np.array_equal(np.diff(t)[:-1], T[:98]),
                                                       np.array_equal(m2[0][:len(t)], t), o2["jitter_local"], list_jitter(t)))
    yg, stg, syg = psola(x, mk, rec, sg, start, T, gains)
    og, mg, rg, _ = guided(yg)
    print("the same with gains 0.85..1.15: %d of %d guided marks moved (by at most %d), jitter_local %.4f for %.4f, "
          "shimmer_local %.4f for %.4f without gains" % ((mg[0][:len(t)] != t).sum(), len(t), np.abs(mg[0][:len(t)] - t).max(),
                                                         og["jitter_local"], list_jitter(t), og["shimmer_local"], o2["shimmer_local"]))
    for c in (98, 154):
        yc, stc, _ = psola(x, mk, rec, sg, *constant(c))
        oc = guided(yc)[0]
        print("constant T = %d: %d marks, F0 %.1f Hz against %.1f" % (c, stc["n_synth"], oc["f0_hz"], FS / c))
    # where it does worse
    rms = lambda v: float(np.sqrt(np.mean(np.asarray(v, dtype=np.float64) ** 2)))  # noqa: E731
    for c in (41, 49, 61, 246, 308):
        yc, stc, syc = psola(x, mk, rec, sg, *constant(c))
        oc, mc, rc, _ = guided(yc)
        a, b = int(mk[0][0]), int(mk[0][rec["n_marks"][0] - 1])
        print("factor %.2f (T = %d): %d marks, the guided track of y reads %.1f Hz for %.1f (%d runs, %d marks); rms inside the "
              "run %.0f for %.0f; samples at zero %.0f %% for %.0f %%"
              % (123.0 / c, c, stc["n_synth"], oc["f0_hz"], FS / c, rc["n_segments"][0], rc["n_marks"][0], rms(yc[a:b]), rms(x[a:b]),
                 100.0 * (yc[a:b] == 0).mean(), 100.0 * (x[a:b] == 0).mean()))
    # an octave error of the track: every second mark only, and a target 20 % up from what that track says
    half = mk.copy()
    k = rec["n_marks"][0]
    half[0, :(k + 1) // 2] = mk[0, :k:2]
    rech = rec.copy()
    rech["n_marks"] = (k + 1) // 2
    sgh = sg.copy()
    sgh["n_marks"][0, 0] = (k + 1) // 2
    yh, sth, _ = psola(x, half, rech, sgh, *constant(205))
    oh = guided(yh)[0]
    print("marks an octave low (every second one), T = 205 (246 / 1.2): %d synthesis marks; the guided track of y reads %.1f Hz: "
          "the wanted %.1f Hz (x's 130.1 * 1.2) is not there, each grain carries two pulses" % (sth["n_synth"], oh["f0_hz"], 130.08 * 1.2))
    g = ps.gaps()
    o, m, r, s = guided(g)
    yg2, stg2, _ = psola(g, m, r, s, *constant(98))
    e0, a1 = int(m[0][s["n_marks"][0, 0] - 1]), int(m[0][s["first_mark_index"][0, 1]])
    print("gaps(), T = 98: %d runs done, %d marks; the %d samples between the runs (and the %d in front, the %d behind) equal x: %s"
          % (stg2["n_runs_done"], stg2["n_synth"], a1 - e0, int(m[0][0]), len(g) - int(m[0][r["n_marks"][0] - 1]),
             np.array_equal(yg2[e0:a1], g[e0:a1]) and np.array_equal(yg2[:int(m[0][0])], g[:int(m[0][0])])))


if __name__ == "__main__":
    main()
