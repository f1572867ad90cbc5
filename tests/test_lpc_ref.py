"""The numpy restatement of the LPC analysis (tests/lpc_ref.py, include/voice_synth.h) on the CPU: it recovers the
formants of the ten tables from their impulse responses and those of synthesised vowels, its int64 autocorrelation
holds at the overflow bound, and the library's host helpers (vs_lpc_window, vs_lpc_frames) equal its formulas.  The GPU
tests compare the device with this restatement, which carries these checks over."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpc_ref as lr  # noqa: E402

TABLES = "aiu1234567"


def _max_pair_error(got, want):
    assert len(got) == len(want), (got, want)
    return max(max(abs(g[0] - w[0]), abs(g[1] - w[1])) for g, w in zip(got, want))


@pytest.mark.parametrize("fs", [16000, 22050, 44100])
def test_table_truth_from_impulse_responses(fs):
    """order-22 LPC of the whole 4096-sample impulse response of 1/A(z) (rectangular window, one centre frame) gives back
    the roots of the table's A: every formant within 2 Hz in f and bw at 16 kHz, the same angle on the unit circle at the
    other rates (2 * fs / 16000 Hz; measured: at most 0.97 Hz at 16 kHz, 2.68 Hz at 44.1 kHz)"""
    worst = 0.0
    for v in TABLES:
        A = vs.vowel_coefficients(v)
        h = lr.impulse_response(A)
        fr = lr.analyse_row(h, fs, window="rectangular", window_s=4096 / fs, hop_s=0, n_formants=20)
        assert len(fr) == 1 and fr[0]["start"] == 0 and fr[0]["status"] == 0
        worst = max(worst, _max_pair_error(fr[0]["formants"], lr.table_formants(A, fs)))
    assert worst <= 2.0 * fs / 16000, worst


# the largest error of a table formant below 4 kHz with bw < 300 Hz, measured with this restatement over the ten tables
# (gain 1, vowel -p 1, F0 110 Hz, 40 ms Hamming centre frame): 92 Hz at 16 kHz, 158 Hz at 22.05 kHz.  Tolerance: 3x.
SPEECH_TOL_HZ = 3 * 158.0


@pytest.mark.parametrize("fs", [16000, 22050])
def test_speech_truth_on_synthesised_vowels(fs):
    lanes = [vs.lane_from_cli((["-r", str(fs)] if fs != 22050 else []) + ["-d", "0.5", "-f", "110"],
                              ["-v", v, "-g", "1", "-p", "1"], 3 + k)[0] for k, v in enumerate(TABLES)]
    pcm = pyoracle.synth(lanes, vs.num_samples(fs, 0.5))
    assert np.abs(pcm).max() < 32767          # unclipped (the default gain 10 clips these vowels)
    errs = []
    for k, v in enumerate(TABLES):
        want = [f for f, b in lr.table_formants(vs.vowel_coefficients(v), fs) if f < 4000 and b < 300]
        fr = lr.analyse_row(pcm[k], fs, window_s=0.040, hop_s=0, n_formants=20)
        assert len(fr) == 1 and fr[0]["status"] == 0
        got = np.array([f for f, b in fr[0]["formants"]])
        errs += [float(np.abs(got - f).min()) for f in want]
    assert len(errs) >= 30 and max(errs) <= SPEECH_TOL_HZ, max(errs)


def test_autocorrelation_at_the_overflow_bound():
    """full-scale alternating input with pre-emphasis (|d| = 65535) and a rectangular window at L = 16384: the int64
    sums equal Python's big integers, and r(0) is within a factor 2 of 2^62"""
    L, order = lr.MAX_WINDOW, 40
    x = np.where(np.arange(L + 1) % 2 == 0, 32767, -32768).astype(np.int16)
    o = lr.opts(order=order, window="rectangular", window_s=L / 16000, hop_s=0, pre_emphasis=1)
    assert lr.frame_plan(16000, len(x), o) == (L, 0, [1])
    r = lr.autocorr(x, 1, L, order, lr.window(L, lr.RECTANGULAR), 1)
    xi = [int(t) for t in x]
    v = [256 * (xi[1 + n] - xi[n]) for n in range(L)]
    assert max(abs(t) for t in v) == 256 * 65535 < 2 ** 24
    big = [sum(v[n] * v[n + k] for n in range(L - k)) for k in range(order + 1)]
    assert r == big
    assert 2 ** 61 < r[0] < 2 ** 62


def test_window_tables_equal_the_restatement():
    Ls = list(range(2, 1200)) + [1323, 1764, 2205, 4096, 4410, 9999, 16383, 16384]
    for L in Ls:
        for kind in (lr.HAMMING, lr.RECTANGULAR):
            assert np.array_equal(vs.lpc_window(L, kind), lr.window(L, kind)), (L, kind)
    for L in (0, 1, 16385):
        with pytest.raises(vs.VsError):
            vs.lpc_window(L)


def test_frame_counts_equal_the_formula():
    rng = np.random.default_rng(5)
    checked = refused = 0
    for _ in range(3000):
        fs = int(rng.choice([8000, 11025, 16000, 22050, 44100, 48000, 96000, int(rng.integers(1000, 200000))]))
        o = lr.opts(order=int(rng.integers(1, 41)), window=int(rng.integers(0, 2)),
                    window_s=float(rng.choice([0.005, 0.02, 0.025, 0.04, rng.uniform(0.0005, 0.4)])),
                    hop_s=float(rng.choice([0.0, 0.005, 0.01, rng.uniform(0.0, 0.05)])),
                    pre_emphasis=int(rng.integers(0, 2)), n_formants=int(rng.integers(0, 21)))
        length = int(rng.integers(0, 40000))
        plan = lr.frame_plan(fs, length, o)
        if plan is None:
            with pytest.raises(vs.VsError):
                vs.lpc_frames(fs, length, **o)
            refused += 1
        else:
            assert vs.lpc_frames(fs, length, **o) == len(plan[2]), (fs, length, o)
            checked += 1
    assert checked > 1000 and refused > 100


def test_options_and_records_match_the_header():
    assert C.sizeof(_ffi.LpcOpts) == 48
    assert vs.LPC_FRAME_DTYPE.itemsize == 32
    o = vs.lpc_opts()
    assert (o.order, o.window, o.pre_emphasis, o.n_formants) == (22, vs.VS_LPC_HAMMING, 0, 5)
    assert (o.window_s, o.hop_s, o.f_lo, o.reserved_) == (0.025, 0.010, 50.0, 0)
    for bad in ({"order": 0}, {"order": 41}, {"n_formants": 21}, {"window": 2}, {"pre_emphasis": 2},
                {"hop_s": -0.01}, {"window_s": 0.0005}, {"window_s": 2.0}, {"f_lo": -1.0}):
        with pytest.raises(vs.VsError):
            vs.lpc_frames(16000, 16000, **bad)


def test_set_coefficients_makes_a_custom_lane():
    lane = vs.default_lane()
    A = vs.vowel_coefficients("a")[:13]
    assert vs.set_coefficients(lane, A) is lane
    assert lane.vowel == 0 and lane.order == 12
    assert list(lane.A[:13]) == list(A) and all(t == 0.0 for t in lane.A[13:])
    for bad in ([1.0], [2.0, 0.5], [1.0] + [0.1] * 41, [1.0, math.nan]):
        with pytest.raises(ValueError):
            vs.set_coefficients(lane, bad)
