"""The numpy restatement of the coefficient tracks (tests/track_ref.py, include/voice_synth.h) on the CPU: in hold mode
with one set it IS the oracle's filter; the library's host helpers (vs_track_reflection, vs_track_glide_sets,
vs_track_from_lpc) equal it bit for bit; glides through the reflection domain stay minimum-phase where direct-form
interpolation does not; and a glide between two tables ends on the formants of its end tables.  The GPU tests compare
the device with this restatement, which carries these checks over."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi, configs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpc_ref as lr  # noqa: E402
import track_ref as tr  # noqa: E402

TABLES = "aiu1234567"
# the tolerance tests/test_lpc_ref.py holds static vowels to (its SPEECH_TOL_HZ)
SPEECH_TOL_HZ = 3 * 158.0
# the worst formant error of TRUTH_PAIRS' plateaus measured with this restatement: 136.1 Hz ('1' -> '7', end plateau); the
# largest |sample| of the three glides 17120
TRUTH_PAIRS = [("a", "i"), ("1", "7"), ("u", "a")]


def _rows(n, n_sets, hop, offset, length, gain=1.0, pre=0.0):
    rows = np.zeros(n, dtype=tr.ROW_DTYPE)
    rows["n_sets"], rows["hop"], rows["offset"], rows["length"] = n_sets, hop, offset, length
    rows["gain"], rows["pre_emphasis"] = gain, pre
    return rows


def test_round2int_equals_the_oracle():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-40000, 40000, 4000), np.arange(-70, 70) / 2.0, np.arange(-70, 70) / 2.0 + 1e-12,
                        np.arange(-70, 70) / 2.0 - 1e-12, [-1e-20, -0.0, 0.0, 32766.5, 32767.5, -32767.5, -32768.5, 1e9,
                                                            -1e9, np.nextafter(1.0, 0), np.nextafter(0.5, 1)]])
    assert np.array_equal(tr.round2int(x), np.array([pyoracle.round2int(v) for v in x], dtype=np.int16))


def test_hold_with_one_set_is_the_oracle_filter():
    n = 4000
    lanes = []
    for k, v in enumerate(TABLES):
        lanes.append(vs.lane_from_cli(["-r", "16000", "-d", "0.5", "-f", str(100 + 2 * k), "-j", "1", "-n", "20"],
                                      ["-v", v, "-g", "%g" % (1 + 0.7 * k), "-p", ["1", "0", "0.37"][k % 3]], 7 + k)[0])
    flow = pyoracle.source(lanes, n)
    want = pyoracle.filter(lanes, flow)
    coefs = np.array([vs.vowel_coefficients(v) for v in TABLES])[:, None, :]
    rows = _rows(10, 1, 1600, 0, n, [l.gain for l in lanes], [l.pre_emphasis for l in lanes])
    got, stat = tr.filter_track(flow, coefs, rows, tr.HOLD)
    assert np.array_equal(got, want) and (stat["status"] == 0).all() and (stat["n_unusable"] == 0).all()
    # a custom set of 40 taps
    A = configs.random_pole_set(40, np.random.default_rng(40))
    wide = [vs.set_coefficients(vs.lane_from_cli(["-r", "16000", "-d", "0.5"], ["-v", "a", "-g", "2", "-p", "0.9"], 3)[0], A)]
    want = pyoracle.filter(wide, flow[:1])
    got, _ = tr.filter_track(flow[:1], A[None, None, :], _rows(1, 1, 7, -5, n, 2.0, 0.9), tr.HOLD)
    assert np.array_equal(got, want) and np.abs(want).max() > 100


def _lib_reflection(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    k = np.zeros(len(A) - 1)
    rc = vs.load().vs_track_reflection(len(A) - 1, A.ctypes.data, k.ctypes.data)
    return rc, k


def _random_reflection_set(order, rng):
    return tr.step_up(rng.uniform(-0.95, 0.95, order) * rng.uniform(0.2, 1.0))


def test_host_helpers_equal_the_restatement_bit_for_bit():
    tabs = [vs.vowel_coefficients(v) for v in TABLES]
    for A in tabs:
        rc, k = _lib_reflection(A)
        want, ok = tr.reflection(A)
        assert rc == 0 and ok and np.array_equal(k, want)
        assert np.array_equal(vs.track_reflection(A), want)
        assert np.abs(tr.step_up(want) - A).max() < 1e-13      # step-down then step-up gives the table back
    for a in range(10):
        for b in range(10):
            if a != b:
                for n_sets in (2, 3, 33):
                    assert np.array_equal(vs.track_glide_sets(tabs[a], tabs[b], n_sets),
                                          tr.glide_sets(tabs[a], tabs[b], n_sets)), (a, b, n_sets)
    rng = np.random.default_rng(11)
    for order in (1, 12, 22, 40):
        for _ in range(20):
            A, B = _random_reflection_set(order, rng), _random_reflection_set(order, rng)
            want, ok = tr.reflection(A)
            assert ok and np.array_equal(vs.track_reflection(A), want)
            assert np.array_equal(vs.track_glide_sets(A, B, 5), tr.glide_sets(A, B, 5))


def test_track_rows_from_lpc_options():
    """the option grid of tests/test_lpc_ref.py's frame-count test, in both modes"""
    rng = np.random.default_rng(5)
    made = refused = 0
    for _ in range(3000):
        fs = int(rng.choice([8000, 11025, 16000, 22050, 44100, 48000, 96000, int(rng.integers(1000, 200000))]))
        o = lr.opts(order=int(rng.integers(1, 41)), window=int(rng.integers(0, 2)),
                    window_s=float(rng.choice([0.005, 0.02, 0.025, 0.04, rng.uniform(0.0005, 0.4)])),
                    hop_s=float(rng.choice([0.0, 0.005, 0.01, rng.uniform(0.0, 0.05)])),
                    pre_emphasis=int(rng.integers(0, 2)), n_formants=int(rng.integers(0, 21)))
        length = int(rng.integers(0, 40000))
        plan = lr.frame_plan(fs, length, o)
        for mode, name in ((tr.HOLD, "hold"), (tr.GLIDE, "glide")):
            want = None if plan is None else tr.from_lpc(plan[0], plan[1], o["pre_emphasis"], len(plan[2]), length, mode)
            if want is None:
                with pytest.raises(vs.VsError):
                    vs.track_from_lpc(fs, length, name, **o)
                refused += 1
            else:
                assert tuple(vs.track_from_lpc(fs, length, name, **o)) == want, (fs, length, o, mode)
                made += 1
    assert made > 1000 and refused > 100
    row = vs.track_from_lpc(16000, 16000, "glide")
    assert tuple(row) == (98, 160, 200, 16000, 1.0, 0.0)
    assert vs.track_from_lpc(16000, 16000, "hold")["offset"] == 120


def _max_radius(A):
    return float(np.abs(np.roots(A)).max())


def test_reflection_glides_stay_minimum_phase_where_direct_form_does_not():
    tabs = [vs.vowel_coefficients(v) for v in TABLES]
    worst = 0.0
    unstable_direct = 0
    for a in range(10):
        for b in range(10):
            if a == b:
                continue
            sets = tr.glide_sets(tabs[a], tabs[b], 33)
            for s in range(33):
                worst = max(worst, _max_radius(sets[s]))
                t = s / 32.0
                if _max_radius(tabs[a] + t * (tabs[b] - tabs[a])) >= 1.0:
                    unstable_direct += 1
    assert worst < 1.0, worst
    assert unstable_direct >= 1


def test_unusable_sets_are_refused_by_the_helpers():
    A = vs.vowel_coefficients("a")
    bad = A.copy()
    bad[5] = np.nan
    out = np.zeros((3, 23))
    lib = vs.load()
    for B in (bad, np.concatenate([[1.0], np.zeros(21), [1.0]]), np.concatenate([[1.0], np.zeros(21), [-1.5]]),
              np.concatenate([[1.0, 2.5], np.zeros(21)])):   # NaN tap; k_22 = 1; k_22 = -1.5; k_1 = 2.5
        assert _lib_reflection(B)[0] == _ffi.VS_ERR_RANGE
        assert not tr.reflection(B)[1]
        assert lib.vs_track_glide_sets(22, A.ctypes.data, B.ctypes.data, 3, out.ctypes.data) == _ffi.VS_ERR_RANGE
        assert lib.vs_track_glide_sets(22, B.ctypes.data, A.ctypes.data, 3, out.ctypes.data) == _ffi.VS_ERR_RANGE
    assert lib.vs_track_glide_sets(22, A.ctypes.data, A.ctypes.data, 1, out.ctypes.data) == _ffi.VS_ERR_RANGE
    assert lib.vs_track_glide_sets(41, A.ctypes.data, A.ctypes.data, 3, out.ctypes.data) == _ffi.VS_ERR_RANGE
    assert lib.vs_track_reflection(0, A.ctypes.data, out.ctypes.data) == _ffi.VS_ERR_RANGE
    assert lib.vs_track_reflection(22, None, out.ctypes.data) == _ffi.VS_ERR_ARG


def test_records_match_the_header():
    assert C.sizeof(_ffi.TrackRow) == 24 and vs.TRACK_ROW_DTYPE.itemsize == 24 and tr.ROW_DTYPE.itemsize == 24
    assert C.sizeof(_ffi.TrackStat) == 8 and vs.TRACK_STAT_DTYPE.itemsize == 8
    assert vs.TRACK_ROW_DTYPE == tr.ROW_DTYPE and vs.TRACK_STAT_DTYPE == tr.STAT_DTYPE
    assert (vs.VS_TRACK_GROUP, vs.VS_TRACK_HOLD, vs.VS_TRACK_GLIDE, vs.VS_TRACK_NO_SET) == (24, 0, 1, 1)
    assert (tr.GROUP, tr.HOLD, tr.GLIDE, tr.NO_SET) == (24, 0, 1, 1)


def truth_anchors(v_from, v_to):
    """11 anchors at hop 1600: three of the start table, five evenly spaced in the reflection domain, three of the end"""
    A, B = vs.vowel_coefficients(v_from), vs.vowel_coefficients(v_to)
    return np.concatenate([[A, A], tr.glide_sets(A, B, 7), [B, B]])


def truth_flow():
    lane = vs.lane_from_cli(["-r", "16000", "-d", "1", "-f", "110"], ["-v", "a"], 3)[0]
    return pyoracle.source([lane], 16000)


def plateau_errors(pcm_row, v_from, v_to, frame):
    """errors (Hz) of the end tables' formants with f < 4 kHz and bw < 300 Hz in the 40 ms Hamming frames centred at
    samples 1600 and 14400; frame(pcm_row, start) -> the frame's formant frequencies"""
    errs = []
    for v, centre in ((v_from, 1600), (v_to, 14400)):
        want = [f for f, b in lr.table_formants(vs.vowel_coefficients(v), 16000) if f < 4000 and b < 300]
        got = np.array(frame(pcm_row, centre - 320))
        errs += [float(np.abs(got - f).min()) for f in want]
    return errs


def _ref_frame(x, start):
    r = lr.autocorr(x, start, 640, 22, lr.window(640), 0)
    A, e, st = lr.levinson(r, 22)
    assert st == 0
    return [f for f, b in lr.formants_of(A, 16000, 20)]


def test_glides_end_on_the_formants_of_their_end_tables():
    flow = truth_flow()
    errs, peak = [], 0
    for v_from, v_to in TRUTH_PAIRS:
        coefs = truth_anchors(v_from, v_to)[None]
        pcm, stat = tr.filter_track(flow, coefs, _rows(1, 11, 1600, 0, 16000, 1.0, 1.0), tr.GLIDE)
        assert stat["status"][0] == 0 and stat["n_unusable"][0] == 0
        peak = max(peak, int(np.abs(pcm.astype(np.int32)).max()))
        errs += plateau_errors(pcm[0], v_from, v_to, _ref_frame)
    print("worst plateau formant error %.1f Hz, largest |sample| %d" % (max(errs), peak))
    assert len(errs) >= 12 and max(errs) <= SPEECH_TOL_HZ, max(errs)
    assert peak < 32767
