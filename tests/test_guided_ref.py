"""The numpy restatement of the guided marks (tests/guided_ref.py, include/voice_synth.h "guided marks") on the CPU: the
constructed signals of the pitch track, the oracle vowels whose one-window estimate is an octave low, and the definition's
own edges.  The GPU tests compare the device with this restatement, which carries these checks over."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import acoustic_ref as ar  # noqa: E402
import guided_ref as gr  # noqa: E402
import pitch_ref as pr  # noqa: E402
import pitch_signals as ps  # noqa: E402


def row(x, **kw):
    """(record, marks, (n_segments, n_marks, n_frames_walked), segs) of one row at 16 kHz"""
    out, mk, rec, sg, _ = gr.track_and_guided(np.asarray(x)[None], 16000, marks=400, segs=8, **kw)
    return out[0], mk[0][:rec["n_marks"][0]], rec[0], sg[0][:rec["n_segments"][0]]


# 1 ---- the constructed signals

def test_glide_every_peak_is_marked():
    x, peaks, periods = ps.glide()
    out, m, rec, sg = row(x)
    peaks = np.asarray(peaks)
    assert rec["n_segments"] == 1 and rec["n_marks"] == 101 == len(peaks)
    assert all(np.abs(m - p).min() <= 1 for p in peaks) and all(np.abs(peaks - q).min() <= 1 for q in m)
    assert 0.009 <= out["jitter_local"] <= 0.011 and out["n_periods"] == 100 and out["status"] == 0
    T = np.diff(m)
    assert T.max() in (219, 220, 221) and T.min() in (79, 80, 81, 82)
    plain, pm = ar.measure(x[None], 16000, marks=400)
    pm = pm[0][pm[0] >= 0]
    assert sum(1 for p in peaks if np.abs(pm - p).min() <= 1) < 90        # the one estimate loses the walk


def test_gaps_two_runs_and_nothing_between():
    g = ps.gaps()
    out, m, rec, sg = row(g)
    assert rec["n_segments"] == 2 and sg["n_marks"].tolist() == [60, 60] and sg["first_mark_index"].tolist() == [0, 60]
    assert (np.diff(m[:60]) == 123).all() and (np.diff(m[60:]) == 123).all() and out["n_periods"] == 118
    assert out["jitter_local"] == 0.0 and out["shimmer_local"] == 0.0
    assert out["status"] & ar.AC_ZERO_AMPLITUDE == 0 and out["status"] == 0
    plain = ar.measure(g[None], 16000)[0]
    assert plain["status"] & ar.AC_ZERO_AMPLITUDE and plain["n_periods"] > 150
    out0, m0, rec0, sg0 = row(g, edge_frames=0)
    T0 = np.concatenate([np.diff(m0[:sg0["n_marks"][0]]), np.diff(m0[sg0["n_marks"][0]:])])
    assert (T0 != 123).any()                                              # the runs reach into the zeros and the noise
    outl, ml, recl, sgl = row(g, segments=gr.MG_LONGEST)
    assert recl["n_segments"] == 1 and np.array_equal(ml, m[:60]) and sgl[0] == sg[0]


def test_octave_trap():
    out, m, rec, sg = row(ps.octave_trap())
    assert rec["n_marks"] == 100 and (np.diff(m) == 160).all() and out["n_periods"] == 99


# 2 ---- the oracle vowels at -s 10, default range

@pytest.fixture(scope="module")
def vowels():
    from oracle import pyoracle
    specs = [(["-d", "1", "-f", "100", "-s", "10"], ["-v", "a"], 300 + k) for k in range(16)]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(22050, d)
    return pyoracle.synth(lanes, ns), pyoracle.source(lanes, ns), 1.0 / lanes[0].gain


def read_guided(x):
    meas, mk, rec, _ = gr.measure_and_glottal(x, 22050)
    out = {"shimmer": float(np.nanmean(meas["shimmer_local"])), "periods": meas["n_periods"].copy()}
    for q in ("oq", "qoq", "naq"):
        out[q] = float(np.nanmean(rec[q]))
    return out


def test_the_guided_chain_on_the_vowels(vowels):
    """The 16 oracle vowels of tests/test_cplpc_ref.py at -s 10, with the DEFAULT f0_min 50 and guided marks (LONGEST) in
    the first pass.  Asserted: status 0 and K 99 in all 16 sets; every err / r0 at most twice the largest the f0_min 70
    chain gives on the same rows; each of the four gaps |closed-phase - flow|, all three signals read through guided
    marks, smaller than IAIF's and within twice tests/test_cplpc_ref.py's PRINTED_GAPS; and the unguided chain at the
    default range has a row whose status is not 0 -- what the feature is for."""
    import cplpc_table
    import inverse_ref as ir
    import lpc_ref as lr
    from test_cplpc_ref import PRINTED_GAPS
    pcm, flow, scale = vowels
    got = gr.closed_phase(pcm, 22050, de_emphasis=1.0, scale=scale)
    s = got["sets"]
    assert (s["status"][:, 0] == 0).all() and (got["meas"]["n_periods"] == 99).all()
    T = np.array([np.diff(m[m >= 0]).mean() for m in got["marks"]])
    assert (np.abs(T - 220.0) < 0.02).all()
    q = s["err"][:, 0] / s["r0"][:, 0]
    narrow = cplpc_table.table(("-s", "10"), 70.0)
    print("err / r0 guided %.1e .. %.1e; f0_min 70 %.1e .. %.1e" % (q.min(), q.max(), narrow["err_over_r0"].min(),
                                                                    narrow["err_over_r0"].max()))
    assert q.max() <= 2 * narrow["err_over_r0"].max()
    L, H, starts = lr.frame_plan(22050, pcm.shape[1], lr.opts())
    n_sets, hop, offset, _ = ir.from_lpc(L, H, 0, len(starts), pcm.shape[1], ir.HOLD)[:4]
    by_iaif = ir.inverse_filter(pcm, got["iaif"]["coefs"], ir.rows_of(len(pcm), n_sets, hop, offset, pcm.shape[1], scale,
                                                                      1.0), ir.HOLD)[0]
    rf, rc, ri = read_guided(flow), read_guided(got["flow"]), read_guided(by_iaif)
    assert (rf["periods"] == 99).all() and (rc["periods"] == 99).all()
    for k in cplpc_table.QUANTITIES:
        gap, other = abs(rc[k] - rf[k]), abs(ri[k] - rf[k])
        print("%-8s flow %.4f closed-phase %.4f gap %.2e, IAIF %.2e" % (k, rf[k], rc[k], gap, other))
        assert gap < other, k
        assert gap <= 2 * PRINTED_GAPS[k], k
    wide = cplpc_table.table(("-s", "10"), 50.0)
    assert (wide["status"] != 0).any() or wide["err_over_r0"].max() > 50 * q.max()
    assert (wide["status"] != 0).any(), wide["status"]


def test_the_flows_read_with_guided_marks(vowels):
    """OQ of the -s 10 flows: 87/220 in every row, as at -s 2, once the marks follow the track; the default read has row 6
    at 440"""
    import cplpc_table
    pcm, flow, scale = vowels
    rg = read_guided(flow)
    calm = cplpc_table.table(("-s", "2"), 50.0)["flow"]["oq"]
    assert abs(rg["oq"] - calm) <= 1e-12 and (rg["periods"] == 99).all()
    plain = cplpc_table.read(flow)
    assert abs(plain["oq"] - calm) > 1e-3
    assert ar.measure(flow, 22050)["p0"][6] == 440


# 3 ---- the definition

def test_one_run_is_the_measurement_on_the_same_marks():
    """vs_measure's formulas (acoustic_ref.measure_row's stage C) on the marks of a single run give the same record"""
    x, peaks, periods = ps.glide()
    frames, _ = pr.track(x[None], 16000)
    r = gr.guided_row(x, 16000, frames[0])
    assert r["guided"][0] == 1
    m, amps = r["runs"][0]
    T = [m[i + 1] - m[i] for i in range(len(m) - 1)]
    K = len(T)
    Tm = float(sum(T)) / float(K)
    loc, rap, ppq = ar._perturbation(T, Tm)
    Am = float(sum(amps)) / float(K)
    sl, apq3, apq5 = ar._perturbation(amps, Am)
    rec = r["rec"]
    assert (rec["jitter_local"], rec["jitter_rap"], rec["jitter_ppq5"]) == (loc, rap, ppq)
    assert (rec["shimmer_local"], rec["shimmer_apq3"], rec["shimmer_apq5"]) == (sl, apq3, apq5)
    assert rec["f0_hz"] == 16000.0 / Tm and rec["n_periods"] == K and rec["first_mark"] == m[0]
    s = gr.summary(16000, r["runs"])
    assert (s["N2"], s["N3"], s["N5"]) == (K - 1, K - 2, K - 4)
    # two runs: no neighbour across the pause
    g = gr.guided_row(ps.gaps(), 16000, pr.track(ps.gaps()[None], 16000)[0][0])
    s = gr.summary(16000, g["runs"])
    assert (s["n_periods"], s["N2"], s["N3"], s["N5"]) == (118, 116, 114, 110)


@pytest.mark.parametrize("H", [160, 161, 1, 2, 7])
def test_the_samples_of_a_run_are_the_frames_of_its_samples(H):
    """a and b against {n : fa <= f(n) <= fb} by brute force, H odd and even"""
    C, F = 480, 9
    length = C + (F - 1) * H + 700
    f = np.array([gr.frame_of(n, C, H, F) for n in range(length)])
    assert f[0] == 0 and f[-1] == F - 1 and (np.diff(f) >= 0).all() and set(f) == set(range(F))
    for fa in range(F):
        for fb in range(fa, F):
            a, b = gr.run_samples(fa, fb, C, H, F, length)
            inside = np.flatnonzero((f >= fa) & (f <= fb))
            assert (a, b) == (inside[0], inside[-1] + 1), (fa, fb)
    a, b = gr.run_samples(2, 3, C, H, F, C + 3 * H)                        # a row that ends inside the run
    assert b == C + 3 * H


def test_a_jumping_track_hits_the_empty_window():
    fs = 16000
    tmin, tmax = ar.lag_bounds(fs)
    x, _ = ps.train([123] * 110, lambda p: 70, lambda c: 9000.0)
    x = x[:12000]
    F = pr.frame_count(len(x), tmax, 160)
    fr = np.zeros(F, pr.FRAME_DTYPE)
    fr["lag"] = np.where(np.arange(F) % 2 == 0, tmin, tmax)
    fr["q"] = 20000
    events = []
    r = gr.guided_row(x, fs, fr, events)
    assert "empty" in events and r["guided"][0] == 1 and r["rec"]["n_periods"] >= 20
    # a fabricated lag outside the range is unvoiced
    fr["lag"] = np.where(np.arange(F) % 2 == 0, tmin - 1, tmax + 1)
    assert gr.guided_row(x, fs, fr)["rec"]["status"] == ar.AC_UNVOICED
    assert gr.guided_row(x[:900], fs, fr)["rec"]["status"] == ar.AC_TOO_SHORT


def test_runs_trim_and_longest():
    v = np.array([1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1], bool)
    assert gr.runs(v, 1, 3, gr.MG_ALL) == [(0, 2), (6, 9), (14, 17)]       # the row's ends are not trimmed
    assert gr.runs(v, 0, 3, gr.MG_ALL) == [(0, 3), (5, 10), (13, 17)]
    assert gr.runs(v, 1, 4, gr.MG_ALL) == [(6, 9), (14, 17)] and gr.runs(v, 1, 4, gr.MG_LONGEST) == [(6, 9)]
    assert gr.runs(v, 2, 1, gr.MG_LONGEST) == [(15, 17)] and gr.runs(v, 16, 1, gr.MG_ALL) == []
    assert gr.runs(np.ones(5, bool), 16, 5, gr.MG_ALL) == [(0, 4)]


def test_the_host_plan_and_defaults():
    """the C ABI's host-only half: defaults, refusals, the row plan against the restatement's"""
    import ctypes as C
    from voice_synth_amd import _ffi
    lib = vs.load()
    o = _ffi.GuidedOpts()
    assert C.sizeof(_ffi.GuidedOpts) == 32 and C.sizeof(_ffi.GuidedRec) == 16 == C.sizeof(_ffi.GuidedSeg)
    assert vs.GUIDED_REC_DTYPE == gr.REC_DTYPE and vs.GUIDED_SEG_DTYPE == gr.SEG_DTYPE
    assert lib.vs_guided_defaults(None) == _ffi.VS_ERR_ARG and lib.vs_guided_defaults(C.byref(o)) == 0
    assert (o.f0_min, o.f0_max, o.polarity, o.segments, o.edge_frames, o.min_frames, o.hop_s) == (50.0, 500.0, 1, 0, 1, 3, 0.010)
    for fs, n in ((16000, 16000), (8000, 700), (22050, 22050), (96000, 6000), (44100, 1324)):
        for kw in (dict(), dict(f0_min=70.0, hop_s=0.005)):
            assert tuple(vs.guided_plan(fs, n, **kw).values()) == gr.plan(fs, n, gr.opts(**kw)), (fs, n, kw)
    for kw, code in ((dict(polarity=0), _ffi.VS_ERR_ARG), (dict(segments=2), _ffi.VS_ERR_ARG),
                     (dict(hop_s=float("inf")), _ffi.VS_ERR_ARG), (dict(f0_min=0.0), _ffi.VS_ERR_ARG),
                     (dict(edge_frames=17), _ffi.VS_ERR_RANGE), (dict(min_frames=0), _ffi.VS_ERR_RANGE),
                     (dict(hop_s=0.0), _ffi.VS_ERR_RANGE), (dict(f0_min=5.0), _ffi.VS_ERR_RANGE)):
        with pytest.raises(vs.VsError) as e:
            vs.guided_plan(16000, 16000, **kw)
        assert e.value.code == code, kw
    assert lib.vs_guided_launch(None, None, None, 0, 0, 0, None, None, None, 0, None, None, 0, None, None, 0) == _ffi.VS_ERR_ARG
    assert lib.vs_guided(None, None, None, None, 0, 0, 0, None, None, 0, None, None, None, 0, None, None, 0) == _ffi.VS_ERR_ARG


def test_the_printed_line():
    rec = np.zeros(1, ar.DTYPE)[0]
    for f in ar.FIELDS:
        rec[f] = np.nan
    g = np.array([(2, 120, 87, 0)], gr.REC_DTYPE)[0]
    assert gr.format_line("f.wav", rec, g) == ar.format_line("f.wav", rec) + " 2 87"
    assert gr.COLUMNS[-2:] == ("segments", "voiced_frames")
