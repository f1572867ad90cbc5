"""The numpy restatement of PSOLA (tests/psola_ref.py, include/voice_synth.h "PSOLA") on the CPU: the four consequences the
definition promises, with the guided marks' restatement on the signals of the pitch track's tests; the definition's own
corners; and the device-free half of the library through ctypes.  The GPU tests compare the device with this restatement,
which carries these checks over."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_ref as gr  # noqa: E402
import pitch_signals as ps  # noqa: E402
import psola_ref as pp  # noqa: E402

Q = pp.Q
INT32_MIN, INT32_MAX = pp.INT32_MIN, pp.INT32_MAX


def guided(x):
    """(record, marks [1][400], rec [1], segs [1][8]) of one row at 16 kHz"""
    out, mk, rec, sg, _ = gr.track_and_guided(np.asarray(x)[None], 16000, marks=400, segs=8)
    return out[0], mk, rec, sg


def run(x, mk, rec, sg, start, T, gain=None, J=None, sp=400, pmin=32, pmax=320, length=None):
    start, T = np.asarray(start, dtype=np.int64), np.asarray(T, dtype=np.int64)
    J = len(start) if J is None else J
    y, st, sy = pp.psola(np.asarray(x)[None], [len(x) if length is None else length], mk, rec, sg, start[None], T[None],
                         None if gain is None else np.asarray(gain)[None], [J], pmin, pmax, sp)
    return y[0], st[0], sy[0]


@pytest.fixture(scope="module")
def train123():
    x, _ = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)
    out, mk, rec, sg = guided(x)
    assert rec["n_segments"][0] == 1 and rec["n_marks"][0] == 100 and out["jitter_local"] == 0.0
    rng = np.random.default_rng(3)
    T = rng.integers(119, 128, 140).astype(np.int32)
    start = (np.cumsum(T) - T).astype(np.int32)
    gains = rng.integers(int(0.85 * Q), int(1.15 * Q) + 1, 140).astype(np.int32)
    return dict(x=x, mk=mk, rec=rec, sg=sg, T=T, start=start, gains=gains)


def list_jitter(t):
    """jitter_local of a list of marks"""
    p = np.diff(np.asarray(t, dtype=np.float64))
    return float(np.abs(np.diff(p)).mean() / p.mean())


# 1 ---- the consequences

@pytest.mark.parametrize("signal", ("glide", "gaps"))
def test_identity(signal):
    x = ps.glide()[0] if signal == "glide" else ps.gaps()
    _, mk, rec, sg = guided(x)
    y, st, sy = run(x, mk, rec, sg, [0], [100], J=0)
    assert np.array_equal(y, x)
    runs, marks = (1, 101) if signal == "glide" else (2, 120)
    assert tuple(st) == (0, runs, runs, marks, 0, 0)
    assert np.array_equal(sy["t"][:marks], mk[0][:marks]) and np.array_equal(sy["k"][:marks], np.arange(marks))
    assert sy["cycle"][:marks].tolist().count(pp.RUN_END) == runs and (sy["gain"][:marks] == Q).all()
    # a target that is there and governs nowhere: every period outside [pmin, pmax]
    y2, st2, _ = run(x, mk, rec, sg, np.arange(300) * 100, [321] * 300)
    assert np.array_equal(y2, x) and tuple(st2) == tuple(st)


def test_the_peak_sample_survives(train123):
    d = train123
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], d["start"], d["T"])
    n = st["n_synth"]
    assert np.array_equal(y[sy["t"][:n]], d["x"][d["mk"][0][sy["k"][:n]]])


def test_imposed_periods_are_read_back(train123):
    d = train123
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], d["start"], d["T"])
    assert tuple(st) == (0, 1, 1, 100, 99, 0)
    t = sy["t"][:100]
    assert np.array_equal(np.diff(t)[:-1], d["T"][:98])
    assert sy["cycle"][:100].tolist() == list(range(99)) + [pp.RUN_END]
    out, mk2, rec2, _ = guided(y)
    assert rec2["n_segments"][0] == 1 and rec2["n_marks"][0] == 100 and np.array_equal(mk2[0][:100], t)
    assert out["jitter_local"] == pytest.approx(list_jitter(t), rel=1e-12)
    assert round(float(out["jitter_local"]), 5) == 0.02207


@pytest.mark.parametrize("T,marks,f0", ((98, 125, 162.9), (154, 80, 103.8)))
def test_constant_targets(train123, T, marks, f0):
    d = train123
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], np.arange(400) * T, [T] * 400)
    assert st["n_synth"] == marks and st["status"] == 0 and st["n_governed"] == marks - 1
    out, _, rec2, _ = guided(y)
    assert rec2["n_marks"][0] == marks and round(float(out["f0_hz"]), 1) == f0
    assert abs(float(out["f0_hz"]) - 16000.0 / T) < 0.5                  # the last gap of the run is the difference


def test_gains_move_amplitudes_and_marks(train123):
    """|y[t_i]| follows the gains.  The guided marks of y: 25 of 100 lie a sample off the synthesis marks (a grain scaled
    against its neighbour tilts the sum next to the peak) and jitter_local reads 0.0257 for the list's 0.0221: up, never
    down.  The figures are the README's; the direction is what is asserted."""
    d = train123
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], d["start"], d["T"], gain=d["gains"])
    assert tuple(st) == (0, 1, 1, 100, 99, 0)
    t, g = sy["t"][:100], sy["gain"][:100].astype(np.int64)
    assert g[0] == Q and g[99] == Q and np.array_equal(g[1:99], d["gains"][1:99])
    peak = d["x"][d["mk"][0][sy["k"][:100]]].astype(np.int64)
    assert np.array_equal(y[t], np.clip((peak * Q * g + (1 << 29)) >> 30, -32768, 32767))
    out, mk2, rec2, _ = guided(y)
    assert rec2["n_marks"][0] == 100
    moved = int((mk2[0][:100] != t).sum())
    assert 0 < moved < 100 and np.abs(mk2[0][:100] - t).max() == 1
    assert out["jitter_local"] > list_jitter(t)
    print("gains: %d marks moved, jitter_local %.4f for %.4f, shimmer_local %.4f" %
          (moved, out["jitter_local"], list_jitter(t), out["shimmer_local"]))


# 2 ---- the corners, on rows made by hand

def ramp(n=4000):
    """a row in which every sample is its own index (mod 30011, signed): a copy that reads the wrong index shows"""
    return ((np.arange(n) * 7) % 30011 - 15000).astype(np.int16)


def hand(marks, runs=None, n=4000, marks_pitch=None):
    """(x, marks [1][mp], rec, segs or None) of a row with those marks; runs: (first, m) pairs"""
    mp = len(marks) if marks_pitch is None else marks_pitch
    mk = np.full((1, mp), -1, dtype=np.int32)
    mk[0, :min(mp, len(marks))] = marks[:mp]
    rec = np.zeros(1, dtype=[("n_segments", "<i4"), ("n_marks", "<i4"), ("n_frames_walked", "<i4"), ("reserved_", "<i4")])
    rec["n_marks"] = len(marks)
    sg = None
    if runs is not None:
        sg = np.zeros((1, len(runs)), dtype=[(k, "<i4") for k in ("first_frame", "n_frames", "first_mark_index", "n_marks")])
        sg["first_mark_index"][0], sg["n_marks"][0] = [r[0] for r in runs], [r[1] for r in runs]
        rec["n_segments"] = len(runs)
    return ramp(n), mk, rec, sg


def test_unusable_runs_are_copied():
    tgt = dict(start=np.arange(100) * 40, T=[40] * 100)
    cases = {
        "one mark": ([500], None),
        "not increasing": ([500, 600, 600, 700], None),
        "a mark at len": ([3800, 3900, 4000], None),
        "a period above the longest lag": ([100, 2149, 2300], None),
        "a negative mark": ([-5, 100, 200], None),
        "marks outside the array": ([100, 200, 300], [(1, 3)]),
        "a negative first": ([100, 200, 300], [(-1, 3)]),
    }
    for what, (marks, runs) in cases.items():
        x, mk, rec, sg = hand(marks, runs)
        y, st, _ = run(x, mk, rec, sg, **tgt)
        assert np.array_equal(y, x), what
        assert tuple(st) == (pp.BAD_RUN | pp.NO_RUN, 1, 0, 0, 0, 0), what
    # a period of exactly the longest lag is usable
    x, mk, rec, sg = hand([100, 2148, 2300])
    assert run(x, mk, rec, sg, **tgt)[1]["n_runs_done"] == 1
    # a run behind an earlier one's end: the second begins AT the first's last mark; the third is fine again
    x, mk, rec, sg = hand([100, 200, 300, 300, 400, 500, 501, 600, 700], [(0, 3), (3, 3), (6, 3)])
    y, st, sy = run(x, mk, rec, sg, **tgt)
    assert tuple(st)[:3] == (pp.BAD_RUN, 3, 2) and np.array_equal(y[300:501], x[300:501])
    assert not np.array_equal(y[100:300], x[100:300]) and not np.array_equal(y[501:700], x[501:700])
    # without segment records the row is one run of n_marks marks, capped at marks_pitch
    x, mk, rec, _ = hand([100, 200, 300, 400], marks_pitch=3)
    y, st, sy = run(x, mk, rec, None, [0], [1], J=0)
    assert tuple(st) == (0, 1, 1, 3, 0, 0) and sy["t"][:3].tolist() == [100, 200, 300]
    # n_segments above seg_pitch and below zero
    x, mk, rec, sg = hand([100, 200, 300], [(0, 3)])
    rec["n_segments"] = 7
    assert run(x, mk, rec, sg, [0], [1], J=0)[1]["n_runs"] == 1
    rec["n_segments"] = -7
    assert tuple(run(x, mk, rec, sg, [0], [1], J=0)[1]) == (pp.NO_RUN, 0, 0, 0, 0, 0)


def test_a_target_with_a_hole():
    """a contiguous stretch, a gap, another stretch: the recording's period inside the gap, a new seek behind it"""
    marks = list(range(100, 3100, 100))
    x, mk, rec, sg = hand(marks)
    start = [0, 90, 180, 270, 360, 1000, 1080, 1160, 1240]
    T = [90, 90, 90, 90, 90, 80, 80, 80, 80]
    y, st, sy = run(x, mk, rec, sg, start, T)
    n = st["n_synth"]
    t, c = sy["t"][:n].tolist(), sy["cycle"][:n].tolist()
    # 100 lies in cycle 1 (90..180); the stretch is then taken one by one, 90 a step, the offset of 10 kept
    assert t[:5] == [100, 190, 280, 370, 460] and c[:4] == [1, 2, 3, 4]
    # cycle 4 ends at 450: from 460 the recording's 100 stands, until a mark falls into 1000..1320
    assert c[4:10] == [-1] * 6 and t[5:11] == [560, 660, 760, 860, 960, 1060]
    assert c[10:14] == [5, 6, 7, 8] and t[11:15] == [1140, 1220, 1300, 1380]
    assert c[14] == -1 and t[15] == 1480 and st["n_governed"] == 8
    assert c[-1] == pp.RUN_END and t[-1] == 3000
    # the indices: the nearest mark at or behind the one before, ties to the smaller
    k = sy["k"][:n].tolist()
    assert k[:5] == [0, 1, 2, 3, 4] and k[t.index(1140)] == 10 and k[t.index(1300)] == 12 and k[t.index(1380)] == 13
    tie = t.index(1480) - 1
    assert t[tie] == 1380


def test_periods_outside_the_range_and_hostile_starts():
    marks = list(range(100, 2100, 100))
    x, mk, rec, sg = hand(marks)
    # T outside [pmin, pmax] inside a contiguous stretch: that mark falls back, the next seeks again
    start, T = [100, 190, 280, 290, 380], [90, 90, 10, 90, 90]
    _, st, sy = run(x, mk, rec, sg, start, T)
    assert sy["cycle"][:4].tolist() == [0, 1, -1, 4] and sy["t"][:5].tolist() == [100, 190, 280, 380, 470]  # 380 is cycle 4's start
    _, st, sy = run(x, mk, rec, sg, [100, 190], [90, 321])
    assert sy["cycle"][:3].tolist() == [0, -1, -1]
    # start decreasing: the prefix scan stops at the first start above the mark
    _, st, sy = run(x, mk, rec, sg, [0, 500, 50, 140], [90, 90, 90, 90])
    assert sy["cycle"][:2].tolist() == [-1, -1]                            # cycle 0 ends at 90; 500 > 100 hides the rest
    _, st, sy = run(x, mk, rec, sg, [50, 40, 140], [60, 70, 90])
    assert sy["cycle"][:2].tolist() == [1, 2] and sy["t"][:3].tolist() == [100, 170, 260]
    # (the largest c is 1, and 100 < 40 + 70; 40 + 70 != 140, so the mark at 170 seeks again and finds cycle 2)
    _, st, sy = run(x, mk, rec, sg, [50, 40, 140], [60, 70, 90], pmin=80)
    assert sy["cycle"][:2].tolist() == [-1, 2] and sy["t"][:3].tolist() == [100, 200, 290]
    # INT32_MIN and INT32_MAX: sums in 64 bits
    _, st, sy = run(x, mk, rec, sg, [INT32_MIN, 100], [320, 100], pmax=320)
    assert sy["cycle"][:2].tolist() == [1, -1]
    _, st, sy = run(x, mk, rec, sg, [INT32_MAX, 100], [100, 100])
    assert st["n_governed"] == 0
    _, st, sy = run(x, mk, rec, sg, [100, INT32_MAX], [INT32_MAX, 100], pmax=2048)
    assert st["n_governed"] == 0
    _, st, sy = run(x, mk, rec, sg, [INT32_MIN], [INT32_MAX], pmax=2048)
    assert st["n_governed"] == 0
    # J negative, and above target_pitch
    _, st, _ = run(x, mk, rec, sg, [100, 190], [90, 90], J=-3)
    assert st["n_governed"] == 0
    _, st, sy = run(x, mk, rec, sg, [100, 190], [90, 90], J=1000)
    assert sy["cycle"][:3].tolist() == [0, 1, -1]


def test_gains():
    marks = list(range(100, 1100, 100))
    x, mk, rec, sg = hand(marks)
    x = np.full(4000, 1000, dtype=np.int16)
    start, T = [100 + 100 * j for j in range(9)], [100] * 9
    gains = [0, 0, 65535, -1, 65536, Q, 1, Q, Q]
    y, st, sy = run(x, mk, rec, sg, start, T, gain=gains)
    n = st["n_synth"]
    assert n == 10 and sy["cycle"][:n].tolist() == [0, 1, 2, -1, -1, 5, 6, 7, 8, pp.RUN_END]
    assert sy["gain"][:n].tolist() == [Q, 0, 65535, Q, Q, Q, 1, Q, Q, Q]  # the first is Q whatever its cycle says
    assert y[200] == 0 and y[300] == (1000 * Q * 65535 + (1 << 29)) >> 30 == 2000 and y[400] == 1000 and y[700] == 0
    assert st["n_clipped"] == 0 and st["n_governed"] == 7


def test_overflow_and_clipping():
    marks = list(range(100, 1100, 100))
    x, mk, rec, sg = hand(marks + [1500, 1600, 1700], [(0, 10), (10, 3)])
    # exactly enough: 10 + 3
    y, st, sy = run(x, mk, rec, sg, [0], [1], J=0, sp=13)
    assert tuple(st) == (0, 2, 2, 13, 0, 0)
    # one short: the second run is copied, the count is what it was; the slots behind are untouched
    fill = np.zeros((1, 12), dtype=pp.MARK_DTYPE)
    fill["t"] = -77
    y, st, sy = pp.psola(x[None], [4000], mk, rec, sg, np.zeros((1, 1), np.int32), np.ones((1, 1), np.int32), None, [0], 32,
                         320, 12, synth=fill)
    assert tuple(st[0]) == (pp.OVERFLOW, 2, 1, 10, 0, 0) and (sy["t"][0, 10:] == -77).all() and np.array_equal(y[0], x)
    # the first run does not fit: the later one is copied too, though it would
    y, st, sy = run(x, mk, rec, sg, [0], [1], J=0, sp=9)
    assert tuple(st) == (pp.OVERFLOW | pp.NO_RUN, 2, 0, 0, 0, 0) and np.array_equal(y, x)
    # at the clamp with gain 65535
    x2 = np.full(4000, 32767, dtype=np.int16)
    x2[::2] = -32768
    start, T = [100 + 100 * j for j in range(9)], [100] * 9
    rec1 = rec.copy()
    rec1["n_marks"] = 10
    y, st, sy = run(x2, mk, rec1, None, start, T, gain=[65535] * 9)
    assert st["n_clipped"] > 300 and y[300] == -32768 and y[301] == 32767   # twice the full scale, clamped
    assert np.array_equal(y[:100], x2[:100]) and np.array_equal(y[1000:], x2[1000:])


def test_lengths():
    marks = list(range(100, 1100, 100))
    x, mk, rec, sg = hand(marks)
    out = np.full((1, 4000), 0x5A5A, dtype=np.int16)
    y, st, _ = pp.psola(x[None], [0], mk, rec, sg, np.zeros((1, 1), np.int32), np.ones((1, 1), np.int32), None, [0], 32, 320,
                        40, out=out)
    assert (y == 0x5A5A).all() and tuple(st[0]) == (pp.BAD_RUN | pp.NO_RUN, 1, 0, 0, 0, 0)
    # len < n_samples: the run's last mark is the row's last sample; a grain that reaches past len reads zeros
    y, st, _ = pp.psola(x[None], [1001], mk, rec, sg, np.arange(0, 2000, 80, dtype=np.int32)[None],
                        np.full((1, 25), 80, np.int32), None, [25], 32, 320, 40, out=out)
    assert (y[0, 1001:] == 0x5A5A).all() and st["n_runs_done"][0] == 1 and y[0, 1000] == x[1000]
    assert np.array_equal(y[0, :100], x[:100])


# 3 ---- the device-free half of the library

def test_defaults_and_refusals_through_ctypes():
    lib = vs.load()
    o = vs.psola_opts()
    assert (o.pmin, o.pmax, list(o.reserved_)) == (32, 320, [0, 0]) and C.sizeof(o) == 16
    assert C.sizeof(vs.PsolaMark) == 16 == vs.PSOLA_MARK_DTYPE.itemsize == pp.MARK_DTYPE.itemsize
    assert C.sizeof(vs.PsolaStat) == 24 == vs.PSOLA_STAT_DTYPE.itemsize == pp.STAT_DTYPE.itemsize
    assert lib.vs_psola_defaults(None) == vs._ffi.VS_ERR_ARG
    assert (vs.VS_PS_BAD_RUN, vs.VS_PS_OVERFLOW, vs.VS_PS_NO_RUN, vs.VS_PS_RUN_END) == (pp.BAD_RUN, pp.OVERFLOW, pp.NO_RUN,
                                                                                        pp.RUN_END)
    # the 16 kHz bounds are the guided plan's
    plan = vs.guided_plan(16000, 16000)
    assert (plan["tmin"], plan["tmax"]) == (o.pmin, o.pmax)
    # no context: refused before anything else is looked at
    p = C.c_void_p(16)
    assert lib.vs_psola_launch(None, None, p, 8, 1, 8, None, p, 4, p, None, 0, p, 4, p, 4, None, 0, p, 4, 4, p, 8, p, p,
                               4) == vs._ffi.VS_ERR_ARG
    assert lib.vs_psola(None, None, p, 8, 1, 8, None, p, 4, p, None, 0, p, p, None, p, 4, p, p, p,
                        4) == vs._ffi.VS_ERR_ARG
