"""The numpy restatement of the acoustic measurement (tests/acoustic_ref.py, include/voice_synth.h) on the CPU: hand-built
pulse trains, the status paths, and the truth the CPU oracle logs for every cycle it synthesises (the GPU's source is
bit-identical to it).  The GPU tests compare the device with this restatement, which carries these checks over.

Tolerances are three times the lane-to-lane spread measured with this restatement (32-lane or 24-lane sets)."""
import math
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402


def pulse_train(periods, amps, n, start=10, w=16):
    """triangular pulses 2*w - 1 samples wide on a zero baseline, peaks at start, start + T_1, ..."""
    x = np.zeros(n, dtype=np.int16)
    pos = start
    marks = []
    for k, a in enumerate(amps):
        if pos >= n:
            break
        for j in range(-w + 1, w):
            if 0 <= pos + j < n:
                x[pos + j] = a * (w - abs(j)) // w
        marks.append(pos)
        if k < len(periods):
            pos += periods[k]
    return x, marks


def hand_perturbation(v):
    v = np.asarray(v, dtype=np.float64)
    m = v.mean()
    loc = np.abs(np.diff(v)).mean() / m
    rap = np.mean([abs(v[i] - v[i - 1:i + 2].mean()) for i in range(1, len(v) - 1)]) / m
    ppq = np.mean([abs(v[i] - v[i - 2:i + 3].mean()) for i in range(2, len(v) - 2)]) / m
    return loc, rap, ppq


def test_pulse_train_gives_back_its_periods_and_amplitudes():
    rng = np.random.default_rng(1)
    periods = list(rng.integers(92, 109, size=60))
    amps = list(rng.integers(9000, 11000, size=61))
    amps[0] = 12000                      # m_0: the highest pulse of [0, tmax)
    x, want = pulse_train(periods, amps, 4000)
    rec, m = ar.measure_row(x, 16000, marks_pitch=1000)
    K = rec["n_periods"]
    assert rec["status"] == 0 and K >= 30 and 92 <= rec["p0"] <= 108
    assert m == want[:K + 1]
    T = periods[:K]
    a = amps[1:K + 1]
    assert rec["f0_hz"] == pytest.approx(16000 / np.mean(T), rel=1e-13)
    jl, jr, jp = hand_perturbation(T)
    assert (rec["jitter_local"], rec["jitter_rap"], rec["jitter_ppq5"]) == pytest.approx((jl, jr, jp), rel=1e-12)
    assert rec["jitter_abs_s"] == pytest.approx(np.abs(np.diff(T)).mean() / 16000, rel=1e-12)
    sl, s3, s5 = hand_perturbation(a)
    assert (rec["shimmer_local"], rec["shimmer_apq3"], rec["shimmer_apq5"]) == pytest.approx((sl, s3, s5), rel=1e-12)
    assert rec["shimmer_db"] == pytest.approx(np.mean(np.abs(20 * np.log10(np.array(a[1:]) / np.array(a[:-1])))), rel=1e-12)
    assert 0 < rec["hnr_db"] < 100


def test_constant_train_has_no_perturbation():
    x, want = pulse_train([100] * 60, [10000] * 61, 4000)
    rec, m = ar.measure_row(x, 16000, marks_pitch=1000)
    assert rec["p0"] == 100 and rec["f0_hz"] == 160.0 and m == want[:rec["n_periods"] + 1]
    for f in ("jitter_local", "jitter_rap", "jitter_ppq5", "shimmer_local", "shimmer_db", "shimmer_apq3", "shimmer_apq5"):
        assert rec[f] == 0.0, f
    assert rec["hnr_db"] == pytest.approx(100.0)   # rho clamped to 1 - 1e-10


def test_status_paths():
    tmin, tmax = ar.lag_bounds(16000)
    assert (tmin, tmax) == (32, 320)
    short = np.ones(3 * tmax + 1, dtype=np.int16)
    rec, m = ar.measure_row(short, 16000, marks_pitch=10)
    assert rec["status"] == ar.AC_TOO_SHORT and m == [] and math.isnan(rec["f0_hz"]) and rec["first_mark"] == -1
    rec, m = ar.measure_row(np.zeros(4000, dtype=np.int16), 16000, marks_pitch=10)
    assert rec["status"] == ar.AC_UNVOICED and m == [] and math.isnan(rec["hnr_db"]) and rec["p0"] == 0
    # F0 320 Hz with f0_min 200 Hz: tmax 80, a 260-sample row holds 4 periods -> no PPQ5 / APQ5
    x, _ = pulse_train([50, 52, 49, 51, 50], [8000, 7000, 7400, 6900, 7100, 7000], 260, start=5, w=8)
    rec, m = ar.measure_row(x, 16000, f0_min=200, marks_pitch=10)
    assert rec["status"] == 0 and 3 <= rec["n_periods"] < 5
    assert math.isnan(rec["jitter_ppq5"]) and math.isnan(rec["shimmer_apq5"])
    assert not math.isnan(rec["jitter_rap"]) and not math.isnan(rec["shimmer_apq3"])
    for bad in ({"f0_min": 5}, {"f0_max": 10000}, {"f0_min": 600}):
        with pytest.raises(ValueError):
            ar.lag_bounds(16000, **bad)


def test_polarity_minus_one_marks_the_minima():
    rng = np.random.default_rng(2)
    periods = list(rng.integers(95, 106, size=40))
    amps = [12000] + list(rng.integers(9000, 11000, size=40))
    x, want = pulse_train(periods, amps, 3000)
    pos, mp = ar.measure_row(x, 16000, marks_pitch=100)
    neg, mn = ar.measure_row(-x, 16000, polarity=-1, marks_pitch=100)
    assert mp == mn == want[:pos["n_periods"] + 1]
    for k in pos:
        assert pos[k] == neg[k] or (isinstance(pos[k], float) and math.isnan(pos[k]) and math.isnan(neg[k])), k


# ---- ground truth on the CPU oracle's flows ----

def flow_lane(fs, f0, jitter=0.0, shimmer=0.0, seed=0):
    fa = (["-r", str(fs)] if fs != 22050 else []) + ["-d", "1", "-f", str(f0), "-g", "%.2f" % (f0 * 125 / 120 + 1)]
    if jitter:
        fa += ["-j", str(jitter)]
    if shimmer:
        fa += ["-s", str(shimmer)]
    lane, _ = vs.lane_from_cli(fa, ["-v", "a"], seed)
    lane.DC = 0.0
    lane.Kvar = 0.0
    return lane


@pytest.mark.parametrize("jitter,want,tol", [(0.5, 0.005, 0.001), (1, 0.010, 0.0015), (2, 0.020, 0.003),
                                             (5, 0.048, 0.0085)])   # (5 %: the reference's rejection trims the tail)
def test_flow_periods_equal_the_cycle_log(jitter, want, tol):
    """fs 22050 / 44100, F0 90..120: the measured periods are the logged T of every full cycle, exactly"""
    jl = []
    for k in range(24):
        fs = (22050, 44100)[k % 2]
        lane = flow_lane(fs, 90 + (7 * k) % 31, jitter=jitter, seed=1000 + k)
        n = vs.num_samples(fs, 1.0)
        flow, recs, ncyc, _ = pyoracle.source_one(lane, n, 400)
        rec, m = ar.measure_row(flow, fs, marks_pitch=1000)
        K = rec["n_periods"]
        assert rec["status"] == 0 and K >= 60
        assert np.array_equal(np.diff(m), recs["T"][:K]), (jitter, k)
        jl.append(rec["jitter_local"])
    assert abs(np.mean(jl) - want) <= tol, np.mean(jl)


@pytest.mark.parametrize("shimmer,tol", [(2, 0.04), (5, 0.055), (10, 0.28)])
def test_flow_shimmer_reads_the_logged_draws(shimmer, tol):
    """F0 100, DC 0: the reference's recursion makes S the relative difference of consecutive amplitudes (fg:293-313),
    so shimmer_local / mean |S| is 1"""
    ratio = []
    for k in range(24):
        fs = (22050, 44100)[k % 2]
        lane = flow_lane(fs, 100, shimmer=shimmer, seed=2000 + k)
        flow, recs, ncyc, _ = pyoracle.source_one(lane, vs.num_samples(fs, 1.0), 400)
        rec, _ = ar.measure_row(flow, fs)
        assert rec["status"] == 0
        ratio.append(rec["shimmer_local"] / np.mean(np.abs(recs["S"][:ncyc])))
    assert abs(np.mean(ratio) - 1.0) <= tol, np.mean(ratio)


# ---- speech (vowel /a/ at 22050 Hz, F0 100) ----

def speech(flowgen_args, vowel_args, seed0, n=32):
    specs = [(["-d", "1", "-f", "100"] + flowgen_args, ["-v", "a"] + vowel_args, seed0 + k) for k in range(n)]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(22050, d)
    return lanes, ns, pyoracle.synth(lanes, ns)


@pytest.mark.parametrize("snr", [10, 20, 30])
def test_speech_hnr_reads_the_vowel_noise(snr):
    _, _, pcm = speech([], ["-n", str(snr)], 100)
    r = ar.measure(pcm, 22050)
    assert np.all(r["status"] == 0)
    assert abs(r["hnr_db"].mean() - snr) <= 0.75, r["hnr_db"].mean()


@pytest.mark.parametrize("jitter,tol", [(1, 0.0018), (2, 0.0036)])
def test_speech_jitter_and_f0(jitter, tol):
    lanes, ns, pcm = speech(["-j", str(jitter)], [], 200)
    r = ar.measure(pcm, 22050)
    assert abs(r["jitter_local"].mean() - jitter / 100) <= tol, r["jitter_local"].mean()
    # the reference's jitter is a random walk of the period (0.8 .. 1.2 P): F0 against the logged periods, not -f
    for i in range(8):
        _, recs, ncyc, _ = pyoracle.source_one(lanes[i], ns, 400)
        assert r["f0_hz"][i] == pytest.approx(22050 / np.mean(recs["T"][:ncyc]), rel=0.01)


def test_speech_shimmer_grows_with_the_set_value():
    """on speech the measure reads about 0.7 x the set shimmer (the previous cycle's ringing dilutes the peaks): only
    its order is asserted"""
    means = [ar.measure(speech(["-s", str(s)], [], 300)[2], 22050)["shimmer_local"].mean() for s in (2, 5, 10)]
    assert means[0] < means[1] < means[2]
    assert 0.4 < means[0] / 0.02 < 1.0
