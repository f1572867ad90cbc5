"""The numpy restatement of PSOLA with a time map (tests/psola_ts_ref.py, include/voice_synth.h "PSOLA with a time map") on
the CPU: the consequences the definition promises, with the guided marks' restatement on the signals of the pitch track's
tests; what a change of duration does to those signals; the definition's own corners; and the device-free half of the
library through ctypes.  The GPU tests compare the device with this restatement, which carries these checks over."""
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
import psola_ts_ref as pt  # noqa: E402

Q = pt.Q


def guided(x):
    """(record, marks [1][400], rec [1], segs [1][8]) of one row at 16 kHz"""
    out, mk, rec, sg, _ = gr.track_and_guided(np.asarray(x)[None], 16000, marks=400, segs=8)
    return out[0], mk, rec, sg


def run(x, mk, rec, sg, len_out, anchors=None, start=(0,), T=(100,), gain=None, J=0, U=80, sp=1200, length=None, W=None,
        pmin=32, pmax=320, width=None, out=None, synth=None):
    """one row through the restatement; anchors: (u, v) pairs, default the two end anchors"""
    N = len(x) if length is None else length
    an = pt.two_anchors(N, len_out) if anchors is None else np.array(anchors, dtype=pt.ANCHOR_DTYPE)
    start, T = np.asarray(start, dtype=np.int64)[None], np.asarray(T, dtype=np.int64)[None]
    y, st, sy = pt.psola_ts(np.asarray(x)[None], [N], len_out if width is None else width, [len_out], mk, rec, sg, start, T,
                            None if gain is None else np.asarray(gain)[None], [J], an[None], [len(an) if W is None else W],
                            pmin, pmax, U, sp, out=out, synth=synth)
    return y[0], st[0], sy[0]


def scaled(N, num, den):
    return (2 * N * num + den) // (2 * den)                  # floor(N * factor + 0.5)


@pytest.fixture(scope="module")
def signals():
    train = ps.train([123] * 100, lambda p: int(0.6 * p), lambda c: 8000.0)[0]
    d = {}
    for name, x in (("glide", ps.glide()[0]), ("gaps", ps.gaps()), ("train", train)):
        out, mk, rec, sg = guided(x)
        d[name] = dict(x=x, mk=mk, rec=rec, sg=sg, out=out)
    assert [int(d[k]["rec"]["n_marks"][0]) for k in ("glide", "gaps", "train")] == [101, 120, 100]
    assert [int(d[k]["rec"]["n_segments"][0]) for k in ("glide", "gaps", "train")] == [1, 2, 1]
    return d


def voiced_runs(sy, n):
    """the records of a row's voiced stretches, a list of index arrays: a voiced record has cycle >= -1, and the record
    that ends a voiced stretch begins an unvoiced one (or is the row's last)"""
    c = sy["cycle"][:n]
    v = np.flatnonzero(c >= -1)
    return [g for g in np.split(v, np.flatnonzero(np.diff(v) > 1) + 1) if len(g)]


# 1 ---- the consequences

@pytest.mark.parametrize("name", ("glide", "gaps", "train"))
def test_the_identity_map_is_psola(signals, name):
    d = signals[name]
    x, N = d["x"], len(d["x"])
    rng = np.random.default_rng(1)
    T = rng.integers(90, 140, 400)
    start = np.cumsum(T) - T
    wy, wst, _ = pp.psola(x[None], [N], d["mk"], d["rec"], d["sg"], start[None], T[None], None, [400], 32, 320, 1200)
    assert wst["n_governed"][0] > 90 and not np.array_equal(wy[0], x)
    for U in (37, 80, 500):
        y, st, sy = run(x, d["mk"], d["rec"], d["sg"], N, start=start, T=T, J=400, U=U)
        assert np.array_equal(y, wy[0]) and st["n_clipped"] == wst["n_clipped"][0] and st["status"] == 0, U
        assert st["n_governed"] == wst["n_governed"][0] and st["n_runs_done"] == wst["n_runs_done"][0]
    # with gains
    gains = rng.integers(Q // 2, 2 * Q, 400)
    wy, wst, _ = pp.psola(x[None], [N], d["mk"], d["rec"], d["sg"], start[None], T[None], gains[None], [400], 32, 320, 1200)
    y, st, _ = run(x, d["mk"], d["rec"], d["sg"], N, start=start, T=T, J=400, gain=gains)
    assert np.array_equal(y, wy[0]) and st["n_clipped"] == wst["n_clipped"][0] and not np.array_equal(y, x)
    # J = 0: the recording
    for U in (2, 80, pt.U_MAX):
        y, st, sy = run(x, d["mk"], d["rec"], d["sg"], N, U=U, sp=N)
        assert np.array_equal(y, x) and st["n_governed"] == 0 and st["n_clipped"] == 0, U
        n = st["n_synth"]
        assert sy["t"][0] == 0 and sy["t"][n - 1] == N and sy["cycle"][n - 1] == pt.RUN_END
        assert (sy["cycle"][:n] != pt.UNVOICED_FLIP).all() and (sy["gain"][:n] == Q).all()


@pytest.mark.parametrize("name", ("glide", "gaps", "train"))
@pytest.mark.parametrize("factor", ((2, 1), (2, 3)))
def test_without_a_governing_cycle_the_voiced_marks_step_by_the_recordings_periods(signals, name, factor):
    d = signals[name]
    N = len(d["x"])
    _, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], scaled(N, *factor))
    n, a = st["n_synth"], d["mk"][0]
    groups = voiced_runs(sy, n)
    assert len(groups) == d["rec"]["n_segments"][0] and st["n_governed"] == 0 and st["status"] == 0
    for g in groups:
        t, k = sy["t"][g], sy["k"][g]
        assert len(g) > 20 and np.array_equal(np.diff(t), a[k[:-1] + 1] - a[k[:-1]])   # PR(k_i): none of them a run's last
        assert (np.diff(k) >= 0).all() and (np.diff(k) <= 2).all()
        assert (np.diff(k) == 0).any() == (factor == (2, 1)) and (np.diff(k) == 2).any() == (factor == (2, 3))


def test_a_contiguous_target_in_output_time_is_read_back(signals):
    d = signals["train"]
    N = len(d["x"])
    rng = np.random.default_rng(3)
    T = rng.integers(119, 128, 260).astype(np.int32)
    start = (np.cumsum(T) - T).astype(np.int32)              # it covers the output, twice the input's length
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], 2 * N, start=start, T=T, J=260)
    n = st["n_synth"]
    (g,) = voiced_runs(sy, n)
    c0 = int(sy["cycle"][g[0]])
    assert c0 >= 0 and start[c0] <= sy["t"][g[0]] < start[c0] + T[c0]
    # (the record that ends the run begins an unvoiced stretch and is no voiced record: the run's last gap lies behind g)
    assert np.array_equal(np.diff(sy["t"][g]), T[c0:c0 + len(g) - 1])
    assert sy["cycle"][g].tolist() == list(range(c0, c0 + len(g))) and st["n_governed"] == len(g) > 190
    out, mk2, rec2, _ = guided(y)
    assert rec2["n_segments"][0] == 1 and abs(int(rec2["n_marks"][0]) - len(g)) <= 2
    assert 0.015 < out["jitter_local"] < 0.03                 # the target's jitter, on a recording that had none


# 2 ---- what a change of duration does

@pytest.mark.parametrize("factor,marks,f0", (((2, 1), 200, 130.25), ((3, 2), 150, 130.10), ((1, 2), 50, 130.08),
                                             ((2, 3), 67, 130.08)))
def test_the_train_keeps_its_pitch(signals, factor, marks, f0):
    d = signals["train"]
    N = len(d["x"])
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], scaled(N, *factor))
    out, _, rec2, _ = guided(y)
    assert st["status"] == 0 and len(y) == scaled(N, *factor)
    assert rec2["n_segments"][0] == 1 and rec2["n_marks"][0] == marks and round(float(out["f0_hz"]), 2) == f0
    assert abs(marks - 100 * factor[0] / factor[1]) <= 2
    assert abs(float(out["f0_hz"]) / float(d["out"]["f0_hz"]) - 1) < 0.01
    if factor == (1, 2):
        assert out["jitter_local"] == 0.0                     # every other cycle, each where it was: exactly periodic


def test_glide_and_gaps_twice_as_long(signals):
    d = signals["glide"]
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], 2 * len(d["x"]))
    out, _, rec2, _ = guided(y)
    assert rec2["n_segments"][0] == 1 and rec2["n_marks"][0] == 202 and abs(202 - 2 * 101) <= 2
    assert abs(float(out["f0_hz"]) / float(d["out"]["f0_hz"]) - 1) < 0.01
    d = signals["gaps"]
    y, st, sy = run(d["x"], d["mk"], d["rec"], d["sg"], 2 * len(d["x"]))
    out, _, rec2, _ = guided(y)
    n = st["n_synth"]
    assert rec2["n_segments"][0] == 2 and rec2["n_marks"][0] == 242 and abs(242 - 2 * 120) <= 2
    assert abs(float(out["f0_hz"]) / float(d["out"]["f0_hz"]) - 1) < 0.01
    assert int((sy["cycle"][:n] == pt.UNVOICED_FLIP).sum()) == 116 and tuple(st) == (0, 2, 2, 469, 0, 0)
    # a flipped mark repeats the k of the mark before it, and no two flipped marks follow each other
    f = np.flatnonzero(sy["cycle"][:n] == pt.UNVOICED_FLIP)
    assert np.array_equal(sy["k"][f], sy["k"][f - 1]) and (np.diff(f) > 1).all() and (sy["cycle"][f - 1] == pt.UNVOICED).all()
    for factor in ((3, 2), (1, 2), (2, 3)):
        y, st, _ = run(d["x"], d["mk"], d["rec"], d["sg"], scaled(len(d["x"]), *factor))
        out, _, rec2, _ = guided(y)
        assert rec2["n_segments"][0] == 2 and abs(int(rec2["n_marks"][0]) - 120 * factor[0] / factor[1]) <= 2, factor
        assert abs(float(out["f0_hz"]) / float(d["out"]["f0_hz"]) - 1) < 0.01, factor


def test_three_anchors(signals):
    """the first half at rate 1, the second three times as long: the first half is the input's"""
    d = signals["train"]
    x, N = d["x"], len(d["x"])
    h = N // 2
    y, st, sy = run(x, d["mk"], d["rec"], d["sg"], h + 3 * (N - h), anchors=[(0, 0), (h, h), (h + 3 * (N - h), N)])
    assert st["status"] == 0 and np.array_equal(y[:h], x[:h]) and len(y) == h + 3 * (N - h)
    n = st["n_synth"]
    (g,) = voiced_runs(sy, n)
    late = g[sy["t"][g] > h + 200]
    assert (np.diff(sy["k"][g[sy["t"][g] < h]]) == 1).all() and (np.diff(sy["k"][late]) == 0).sum() > 90
    out, _, rec2, _ = guided(y)
    assert rec2["n_segments"][0] == 1 and abs(int(rec2["n_marks"][0]) - 200) <= 2
    assert abs(float(out["f0_hz"]) / float(d["out"]["f0_hz"]) - 1) < 0.01


# 3 ---- the corners, on rows made by hand

def ramp(n=4000):
    return ((np.arange(n) * 7) % 30011 - 15000).astype(np.int16)


def hand(marks, runs=None, n=4000):
    mk = np.array([marks], dtype=np.int32)
    rec = np.zeros(1, dtype=[("n_segments", "<i4"), ("n_marks", "<i4"), ("n_frames_walked", "<i4"), ("reserved_", "<i4")])
    rec["n_marks"] = len(marks)
    sg = None
    if runs is not None:
        sg = np.zeros((1, len(runs)), dtype=[(k, "<i4") for k in ("first_frame", "n_frames", "first_mark_index", "n_marks")])
        sg["first_mark_index"][0], sg["n_marks"][0] = [r[0] for r in runs], [r[1] for r in runs]
        rec["n_segments"] = len(runs)
    return ramp(n), mk, rec, sg


def test_the_map_and_its_inverse():
    mp = ([0, 10, 20, 50], [0, 30, 30, 40])                   # fast, frozen, slow
    assert [pt.M(mp, n) for n in (0, 1, 9, 10, 19, 20, 23, 49)] == [0, 3, 27, 30, 30, 30, 31, 39]
    assert [pt.Minv(mp, p) for p in (0, 1, 3, 4, 30, 31, 39, 40)] == [0, 1, 1, 2, 10, 23, 47, 50]
    for p in range(41):                                      # the definition, searched
        want = next((n for n in range(50) if pt.M(mp, n) >= p), 50) if 0 < p < 40 else (0 if p == 0 else 50)
        assert pt.Minv(mp, p) == want, p
    frozen_end = ([0, 10, 50], [0, 40, 40])
    assert pt.Minv(frozen_end, 40) == 50 and pt.Minv(frozen_end, 39) == 10    # Minv(len) is len_out by definition
    # 64 bits: (n - u_j) * (v_{j+1} - v_j) beyond 2^31
    big = ([0, 2**31 - 1], [0, 2**31 - 2])
    assert pt.M(big, 2**31 - 2) == 2**31 - 3 and pt.Minv(big, 2**31 - 3) == 2**31 - 2


def test_unvoiced_marks():
    assert pt.unvoiced_marks(0, 120, 80) == [0, 120] and pt.unvoiced_marks(0, 121, 80) == [0, 80, 121]
    assert pt.unvoiced_marks(5, 6, 80) == [5, 6] and pt.unvoiced_marks(0, 281, 80) == [0, 80, 160, 240, 281]
    assert pt.unvoiced_marks(0, 280, 80) == [0, 80, 160, 280] and pt.unvoiced_marks(0, 7, 2) == [0, 2, 4, 7]
    for U in (2, 3, 80, pt.U_MAX):                           # every interval at or below VS_AC_MAX_LAG
        for gap in (1, U, U + U // 2, U + U // 2 + 1, 5 * U + 1, 3000):
            d = np.diff(pt.unvoiced_marks(10, 10 + gap, U))
            assert d.min() >= 1 and d.max() <= min(pt.MAX_LAG, U + U // 2) and (d[:-1] == U).all(), (U, gap)
            assert len(d) == 1 or U // 2 < d[-1] <= U + U // 2


def test_every_way_a_map_can_be_invalid():
    x, mk, rec, sg = hand(list(range(100, 1100, 100)))
    good = [(0, 0), (1000, 2000), (5000, 4000)]
    assert run(x, mk, rec, sg, 5000, anchors=good)[1]["status"] == 0
    bad = {
        "one anchor": (good, 1), "no anchor": (good, 0), "a negative count": (good, -1), "more than map_pitch": (good, 4),
        "u_0": ([(1, 0), (1000, 2000), (5000, 4000)], 3), "v_0": ([(0, 1), (1000, 2000), (5000, 4000)], 3),
        "u_last": ([(0, 0), (1000, 2000), (4999, 4000)], 3), "v_last": ([(0, 0), (1000, 2000), (5000, 3999)], 3),
        "v_last above": ([(0, 0), (1000, 2000), (5000, 4001)], 3), "u repeats": ([(0, 0), (1000, 2000), (1000, 2500), (5000, 4000)], 4),
        "u falls": ([(0, 0), (1000, 2000), (999, 2500), (5000, 4000)], 4), "v falls": ([(0, 0), (1000, 2000), (2000, 1999), (5000, 4000)], 4),
    }
    fill = np.full((1, 5003), 0x5A5A, np.int16)
    marks = np.zeros((1, 50), dtype=pt.MARK_DTYPE)
    marks["t"] = -77
    for what, (an, W) in bad.items():
        y, st, sy = run(x, mk, rec, sg, 5000, anchors=an, W=W, width=5003, out=fill, synth=marks, sp=50)
        assert tuple(st) == (pt.BAD_MAP | pt.NO_RUN, 1, 0, 0, 0, 0), what
        assert (y[:5000] == 0).all() and (y[5000:] == 0x5A5A).all() and (sy["t"] == -77).all(), what
    # v may repeat (a frozen piece), u may not; len_out = 0 has no valid map, whatever the anchors
    assert run(x, mk, rec, sg, 5000, anchors=[(0, 0), (1000, 2000), (2000, 2000), (5000, 4000)])[1]["status"] == 0
    y, st, _ = run(x, mk, rec, sg, 0, width=3, out=fill[:, :3])
    assert st["status"] == pt.BAD_MAP | pt.NO_RUN and (y == 0x5A5A).all()


def test_short_outputs_short_inputs_and_stretches_without_marks():
    x, mk, rec, sg = hand([100, 200, 300, 1500, 1600, 1700, 3900, 3950, 3999], [(0, 3), (3, 3), (6, 3)])
    # seven stretches cover [0, 4000]; in an output of 1 or 2 samples every sample is a mark, each a boundary: of the gap
    # in front of the first run, and (Minv(p) = 2 for p > 2000) of the gap between the second run and the third
    for len_out in (1, 2):
        y, st, sy = run(x, mk, rec, sg, len_out)
        assert tuple(st) == (0, 3, 3, len_out + 1, 0, 0) and sy["t"][:len_out + 1].tolist() == list(range(len_out + 1))
        assert sy["cycle"][:len_out + 1].tolist() == [pt.UNVOICED] * len_out + [pt.RUN_END] and y[0] == x[0]
    assert y[1] == x[1700]                                   # the left grain of the boundary at 1: the gap's first mark
    # 40 samples: Minv is p // 100 rounded up; the runs 100..300 and 1500..1700 get two samples each, 3900..3999 one
    y, st, sy = run(x, mk, rec, sg, 40)
    n = st["n_synth"]
    t = sy["t"][:n].tolist()
    assert t[0] == 0 and t[-1] == 40 and (np.diff(t) > 0).all() and st["status"] == 0 and st["n_runs_done"] == 3
    assert {1, 3, 15, 17, 39}.issubset(t)
    # heavier: 7 samples for 4000.  Stretches without marks: every record is a boundary, and a boundary behind such a
    # stretch reads its right grain where the stretch before it ended and its left grain where the next begins
    recs, stt = pt.plan_row(4000, 7, mk[0], [(0, 3), (3, 3), (6, 3)], ([0, 7], [0, 4000]), 80, [0], [100], None, 0, 32, 320, 50)
    assert [r["t"] for r in recs] == sorted({pt.Minv(([0, 7], [0, 4000]), p) for p in (0, 100, 300, 1500, 1700, 3900, 3999, 4000)})
    assert any(r["al"] != r["ar"] for r in recs) and recs[-1]["cycle"] == pt.RUN_END
    # len = 0: no stretch, no marks, silence; the map (0,0) -> (len_out, 0) is valid
    y, st, sy = run(x, mk, rec, sg, 5, length=0, width=8, out=np.full((1, 8), 0x5A5A, np.int16))
    assert tuple(st) == (pt.BAD_RUN | pt.NO_RUN, 3, 0, 0, 0, 0) and y.tolist() == [0] * 5 + [0x5A5A] * 3
    # a run that begins at 0 has no gap in front of it; a row without a run is one unvoiced stretch
    x, mk, rec, sg = hand([0, 100, 200])
    _, st, sy = run(x, mk, rec, sg, 8000)
    assert sy["cycle"][0] == -1 and sy["k"][0] == 0 and st["n_runs_done"] == 1
    x, mk, rec, sg = hand([500])
    y, st, sy = run(x, mk, rec, sg, 8000)
    n = st["n_synth"]
    assert st["status"] == pt.BAD_RUN | pt.NO_RUN and n == 101 and (sy["cycle"][:n - 1] <= pt.UNVOICED).all()
    assert sy["cycle"][:4].tolist() == [pt.UNVOICED, pt.UNVOICED_FLIP, pt.UNVOICED, pt.UNVOICED_FLIP] and sy["k"][:4].tolist() == [0, 0, 1, 1]
    # a flipped grain reads backwards from its mark: at its own instant it is the mark's sample, a step on the one before it
    i = 1
    assert y[sy["t"][i]] == x[80 * sy["k"][i]] and y[sy["t"][i] + 1] != x[80 * sy["k"][i] + 1]


def test_frozen_pieces():
    x, mk, rec, sg = hand(list(range(100, 3100, 100)))
    # 1000 output samples all at input instant 1500, inside the run: the mark at 1500 is repeated, not flipped (voiced)
    y, st, sy = run(x, mk, rec, sg, 5000, anchors=[(0, 0), (1500, 1500), (2500, 1500), (5000, 4000)])
    n = st["n_synth"]
    t, k = sy["t"][:n], sy["k"][:n]
    held = (t >= 1500) & (t < 2500) & (sy["cycle"][:n] == -1)
    assert held.sum() == 10 and (k[held] == 14).all() and st["status"] == 0
    assert np.array_equal(y[:1400], x[:1400])
    # frozen at the start and at the end, in unvoiced stretches: the first and the last grain alternate
    y, st, sy = run(x, mk, rec, sg, 6000, anchors=[(0, 0), (1000, 0), (5000, 4000), (6000, 4000)])
    n = st["n_synth"]
    c, k = sy["cycle"][:n], sy["k"][:n]
    assert c[:6].tolist() == [pt.UNVOICED, pt.UNVOICED_FLIP] * 3 and (k[:12] == 0).all()
    assert c[n - 6:n - 1].tolist() in ([pt.UNVOICED, pt.UNVOICED_FLIP, pt.UNVOICED, pt.UNVOICED_FLIP, pt.UNVOICED],
                                       [pt.UNVOICED_FLIP, pt.UNVOICED, pt.UNVOICED_FLIP, pt.UNVOICED, pt.UNVOICED_FLIP])
    assert sy["t"][n - 1] == 6000 and (np.diff(sy["t"][:n]) > 0).all()


def test_overflow_and_the_unvoiced_period_at_both_limits():
    x, mk, rec, sg = hand(list(range(100, 1100, 100)))
    _, st, sy = run(x, mk, rec, sg, 4000, sp=60)
    n = int(st["n_synth"])
    assert st["status"] == 0 and n == 1 + 10 + 36 + 1 == 48                  # 0 | 100..1000 | 1080..3880 | 4000
    fill = np.zeros((1, n - 1), dtype=pt.MARK_DTYPE)
    fill["t"] = -77
    out = np.full((1, 4004), 0x5A5A, np.int16)
    y, st, sy = run(x, mk, rec, sg, 4000, sp=n, width=4004, out=out)
    assert st["n_synth"] == n and st["status"] == 0 and np.array_equal(y[:4000], x)
    y, st, sy = run(x, mk, rec, sg, 4000, sp=n - 1, synth=fill, width=4004, out=out)
    assert tuple(st) == (pt.OVERFLOW, 1, 1, 0, 0, 0) and (sy["t"] == -77).all()
    assert (y[:4000] == 0).all() and (y[4000:] == 0x5A5A).all()
    # U = 2: marks every 2 samples outside the run; U = 1365: none fits the gaps of 100 and 3000 but one
    y, st, sy = run(x, mk, rec, sg, 4000, U=2, sp=4000)
    assert st["n_synth"] == 50 + 1 + 9 + 1500 == 1560 and np.array_equal(y, x)
    y, st, sy = run(x, mk, rec, sg, 4000, U=pt.U_MAX, sp=4000)
    n = st["n_synth"]
    assert sy["t"][:n].tolist() == [0] + list(range(100, 1100, 100)) + [1000 + 1365, 4000] and np.array_equal(y, x)
    assert np.diff(sy["t"][:n]).max() == 1635 <= pt.MAX_LAG
    with pytest.raises(AssertionError):
        run(x, mk, rec, sg, 4000, U=pt.U_MAX + 1)
    with pytest.raises(AssertionError):
        run(x, mk, rec, sg, 4000, U=1)


def test_hostile_rows_keep_the_chain():
    """drawn maps, runs and periods: the first mark is 0, the last len_out, t strictly increases, no interval exceeds
    3 * VS_AC_MAX_LAG / 2, and the last record alone ends the row"""
    rng = np.random.default_rng(11)
    seen = 0
    for trial in range(120):
        N = int(rng.integers(0, 3001))
        len_out = int(rng.integers(1, 6002))
        W = min(int(rng.integers(2, 6)), len_out + 1)
        u = [0] + sorted(int(q) for q in rng.choice(np.arange(1, max(2, len_out)), W - 2, replace=False)) + [len_out]
        v = [0] + sorted(int(q) for q in rng.integers(0, N + 1, W - 2)) + [N]
        if W > 2 and rng.random() < 0.4:
            v[1] = v[0] if rng.random() < 0.5 else v[2]
        marks, at = [], int(rng.integers(0, 300))
        runs = []
        for r in range(int(rng.integers(0, 4))):
            m = int(rng.integers(1, 30))
            run_ = at + np.concatenate([[0], np.cumsum(rng.integers(1, 300, m - 1))]) if m > 1 else np.array([at])
            runs.append((len(marks) - (1 if rng.random() < 0.1 and marks else 0), m))
            marks += [int(q) for q in run_]
            at = marks[-1] + int(rng.integers(-50, 500))
        x, mk, rec, sg = hand(marks or [0], runs, n=max(N, 1))
        U = int(rng.choice([2, 3, 17, 80, 500, pt.U_MAX]))
        T = rng.integers(20, 400, 50)
        y, st, sy = run(x, mk, rec, sg, len_out, anchors=list(zip(u, v)), start=np.cumsum(T) - T, T=T, J=50, U=U, sp=len_out + 2,
                        length=N)
        if N == 0:
            assert st["n_synth"] == 0 and (y == 0).all()
            continue
        n = st["n_synth"]
        t = sy["t"][:n]
        assert st["status"] & (pt.BAD_MAP | pt.OVERFLOW) == 0 and t[0] == 0 and t[-1] == len_out, trial
        assert (np.diff(t) > 0).all() and np.diff(t).max() <= 3 * pt.MAX_LAG // 2, trial
        assert (sy["cycle"][:n] == pt.RUN_END).sum() == 1 and sy["cycle"][n - 1] == pt.RUN_END and (sy["gain"][:n] >= 0).all()
        seen += 1
    assert seen > 100


# 4 ---- the device-free half of the library

def test_defaults_and_refusals_through_ctypes():
    lib = vs.load()
    o = vs.psola_ts_opts()
    assert (o.pmin, o.pmax, o.unvoiced_period, o.reserved_) == (32, 320, 80, 0) and C.sizeof(o) == 16
    assert C.sizeof(vs.PsolaAnchor) == 8 == vs.PSOLA_ANCHOR_DTYPE.itemsize == pt.ANCHOR_DTYPE.itemsize
    assert lib.vs_psola_ts_defaults(None) == vs._ffi.VS_ERR_ARG
    assert (vs.VS_PS_BAD_MAP, vs.VS_PS_UNVOICED, vs.VS_PS_UNVOICED_FLIP) == (pt.BAD_MAP, pt.UNVOICED, pt.UNVOICED_FLIP)
    assert pt.U_MAX == 1365 and vs.psola_ts_opts(unvoiced_period=7).unvoiced_period == 7
    an, w = vs.psola_two_anchors([100, 7], [250, 3], 4)
    assert an.shape == (2, 4) and w.tolist() == [2, 2] and an[1].tolist()[:2] == [(0, 0), (3, 7)]
    # no context: refused before anything else is looked at
    p = C.c_void_p(16)
    assert lib.vs_psola_ts_launch(None, None, p, 8, 1, 8, None, p, 4, p, None, 0, p, 4, p, 4, None, 0, p, 4, 4, p, p, 2, p, 8,
                                  8, None, p, p, 4) == vs._ffi.VS_ERR_ARG
    assert lib.vs_psola_ts(None, None, p, 8, 1, 8, None, p, 4, p, None, 0, p, p, None, p, 4, p, p, 2, p, 8, None, p, p,
                           4) == vs._ffi.VS_ERR_ARG
    # the check itself: every refusal, in the order ARG, UNSUPPORTED, RANGE
    check = lib.vs_psola_ts_check
    check.restype = C.c_int
    check.argtypes = [C.POINTER(vs.PsolaTsOpts)] + [C.c_size_t] * 4 + [C.c_int] + [C.c_size_t] * 3 + [C.c_int] + \
        [C.c_size_t] * 7 + [C.POINTER(vs.PsolaTsOpts)]
    A, UNS, R, OK = vs._ffi.VS_ERR_ARG, vs._ffi.VS_ERR_UNSUPPORTED, vs._ffi.VS_ERR_RANGE, 0
    names = ("pitch", "n_lanes", "n_samples", "marks_pitch", "has_segs", "seg_pitch", "start_stride", "period_stride", "has_gain",
             "gain_stride", "count_stride", "target_pitch", "map_pitch", "out_pitch", "out_samples", "synth_pitch")
    good = dict(pitch=100, n_lanes=1, n_samples=100, marks_pitch=1, has_segs=0, seg_pitch=0, start_stride=4, period_stride=4,
                has_gain=0, gain_stride=0, count_stride=4, target_pitch=1, map_pitch=2, out_pitch=300, out_samples=300,
                synth_pitch=2)

    def ck(opts=None, **kw):
        a = dict(good, **kw)
        r = vs.PsolaTsOpts()
        return check(None if opts is None else C.byref(opts), *[a[k] for k in names], C.byref(r)), r
    rc, r = ck()
    assert rc == OK and (r.pmin, r.pmax, r.unvoiced_period) == (32, 320, 80)
    for kw in (dict(n_lanes=0), dict(n_samples=0), dict(out_samples=0), dict(marks_pitch=0), dict(target_pitch=0),
               dict(pitch=99), dict(out_pitch=299), dict(synth_pitch=1), dict(map_pitch=1), dict(map_pitch=0),
               dict(has_segs=1, seg_pitch=0), dict(start_stride=2), dict(period_stride=6), dict(count_stride=0),
               dict(has_gain=1, gain_stride=3)):
        assert ck(**kw)[0] == A, kw
    assert ck(has_gain=0, gain_stride=7)[0] == OK and ck(has_segs=1, seg_pitch=1)[0] == OK
    o = vs.psola_ts_opts()
    o.reserved_ = 1
    assert ck(o)[0] == A
    big = 1 << 31
    for kw in (dict(pitch=big), dict(n_lanes=big), dict(marks_pitch=big), dict(target_pitch=big), dict(map_pitch=big),
               dict(out_pitch=big), dict(synth_pitch=big), dict(pitch=big, n_samples=big), dict(out_pitch=big, out_samples=big),
               dict(n_lanes=1 << 20, out_samples=1 << 22, out_pitch=1 << 22)):
        assert ck(**kw)[0] == UNS, kw
    assert ck(n_lanes=1 << 20, out_samples=1 << 21, out_pitch=1 << 21)[0] == OK
    for kw, want in ((dict(pmin=2), OK), (dict(pmin=1), R), (dict(pmin=321), R), (dict(pmax=2048), OK), (dict(pmax=2049), R),
                     (dict(unvoiced_period=2), OK), (dict(unvoiced_period=1), R), (dict(unvoiced_period=1365), OK),
                     (dict(unvoiced_period=1366), R), (dict(unvoiced_period=-5), R)):
        assert ck(vs.psola_ts_opts(**kw))[0] == want, kw
    # an ARG fault is named before an UNSUPPORTED one, and that before a RANGE fault
    assert ck(vs.psola_ts_opts(pmin=0), synth_pitch=1, pitch=big)[0] == A
    assert ck(vs.psola_ts_opts(pmin=0), pitch=big)[0] == UNS
    # the overlap of the input's and the output's rows, and the row records
    ov = lib.vs_psola_ts_overlap
    ov.restype = C.c_int
    ov.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
    assert ov(1000, 10, 8, 1000, 10, 8, 2) == 1 and ov(1000, 10, 8, 1036, 20, 16, 2) == 0 and ov(1000, 10, 8, 1034, 20, 16, 2) == 1
    assert ov(1072, 10, 8, 1000, 20, 16, 2) == 0 and ov(1070, 10, 8, 1000, 20, 16, 2) == 1
    fill = lib.vs_psola_ts_fill
    fill.restype = C.c_int
    fill.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
    rows = np.zeros((3, 2), np.int32)
    ln, lo = np.array([0, 50, 100], np.int32), np.array([300, 0, 1], np.int32)
    assert fill(ln.ctypes.data, lo.ctypes.data, 3, 100, 300, rows.ctypes.data) == OK and rows.tolist() == [[0, 300], [50, 0], [100, 1]]
    assert fill(None, None, 3, 100, 300, rows.ctypes.data) == OK and rows.tolist() == [[100, 300]] * 3
    for bad_ln, bad_lo in (([0, 101, 1], [1, 1, 1]), ([0, -1, 1], [1, 1, 1]), ([1, 1, 1], [1, 301, 1]), ([1, 1, 1], [1, 1, -1])):
        a, b_ = np.array(bad_ln, np.int32), np.array(bad_lo, np.int32)
        assert fill(a.ctypes.data, b_.ctypes.data, 3, 100, 300, rows.ctypes.data) == R
