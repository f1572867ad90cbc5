"""The numpy restatement of the coefficient tracks (tests/track_ref.py, include/voice_synth.h) on the CPU: in hold mode
with one set it IS the oracle's filter; the library's host helpers (vs_track_reflection, vs_track_glide_sets,
vs_track_from_lpc) equal it bit for bit; glides through the reflection domain stay minimum-phase where direct-form
interpolation does not; and a glide between two tables ends on the formants of its end tables.  The GPU tests compare
the device with this restatement, which carries these checks over.

The second half holds the FMA form of the restatement (libm's fma against rational arithmetic; equal to the exact form
where every product is exact) and builds the cases of tests/test_gpu_track_hostile.py -- saturation far past int32,
unstable sets in hold mode, the sets vs_lpc makes of recordings -- with the conditions under which those comparisons
mean something, asserted from the restatement alone.  The GPU tests take the cases and the expected bytes from here."""
import ctypes as C
import fractions
import functools
import itertools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi, configs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_signals as hs  # noqa: E402
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


# ---- the FMA form of the restatement ---------------------------------------------------------------------------------

def test_libm_fma_is_the_exactly_rounded_one():
    """24000 triples, half of them with c within a few ulps of -a*b (where a product rounded on its own loses every
    bit of the result), against fractions.Fraction: float() of a Fraction rounds to nearest even once"""
    rng = np.random.default_rng(53)
    n = 12000
    a = rng.uniform(-2.0, 2.0, 2 * n) * 2.0 ** rng.integers(-200, 200, 2 * n)
    b = rng.uniform(-2.0, 2.0, 2 * n) * 2.0 ** rng.integers(-200, 200, 2 * n)
    c = rng.uniform(-2.0, 2.0, 2 * n) * 2.0 ** rng.integers(-400, 400, 2 * n)
    near = -(a[n:] * b[n:])
    for _ in range(3):                          # 0..3 ulps away, either side
        near = np.where(rng.integers(0, 2, n) == 1, np.nextafter(near, rng.choice([-np.inf, np.inf], n)), near)
    c[n:] = near
    a[:50], b[:50] = rng.integers(-9, 10, 50), rng.integers(-9, 10, 50)       # exact products, zeros among them
    got = tr.fma(a, b, c)
    F = fractions.Fraction
    want = np.array([float(F(float(x)) * F(float(y)) + F(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert (got[n:] != a[n:] * b[n:] + c[n:]).sum() > n // 2     # ... and the unfused form is another function there


def test_fma_form_with_exact_products_is_the_exact_form():
    """integer taps, gains and flows: every product and sum below is an integer under 2^53, so nothing rounds, and the
    two partial sums of the FMA form add up to the one sum of the exact form (before the clamp too: extremes)"""
    rng = np.random.default_rng(54)
    n, R, K = 50, 40, 3            # 50 samples: both halves of the wide window, and Fibonacci growth stays under 2^45
    flow = rng.integers(-9, 10, (R, n)).astype(np.int16)
    clamped = False
    for order in (1, 2, 3, 22, 23, 40):
        coefs = np.zeros((R, K, order + 1))
        coefs[..., 0] = 1.0
        for r in range(R):
            for k in range(K):                   # two taps of +-1: the state grows like a Fibonacci sequence at most
                coefs[r, k, rng.integers(1, order + 1, 2)] = rng.choice([-1.0, 1.0], 2)
        gains = rng.integers(1, 4, (R, K)).astype(np.float64)
        rows = _rows(R, K, rng.integers(1, 30, R), rng.integers(-10, 30, R), rng.integers(0, n + 1, R),
                     rng.integers(1, 5, R), rng.integers(0, 2, R))
        for g in (None, gains):
            pe, xe, pf, xf = [], [], [], []
            exact = tr.filter_track(flow, coefs, rows, tr.HOLD, g, state_max=pe, extremes=xe)
            fused = tr.filter_track(flow, coefs, rows, tr.HOLD, g, state_max=pf, extremes=xf, arith="fma")
            assert pe[0] < 2.0 ** 45 and pe == pf, (order, pe)
            assert np.array_equal(exact[0], fused[0]) and np.array_equal(exact[1], fused[1])
            assert np.array_equal(xe[0][0], xf[0][0]) and np.array_equal(xe[0][1], xf[0][1])
            assert np.abs(exact[0]).max() > 9
            clamped = clamped or xe[0][1].max() > 32767
    assert clamped


# ---- the cases of tests/test_gpu_track_hostile.py --------------------------------------------------------------------

HOSTILE_N = 1210          # 50 groups of 24, one whole vector of 8 and two scalar samples
HOSTILE_FS = 16000
INT32 = 2.0 ** 31
STATE_FINITE = 1e300
SAT_ORDERS = (1, 2, 12, 22, 23, 40)
SAT_K = 5
# every (row gain, pre-emphasis, hop, offset), eight draws of sets each: 960 rows
SAT_COMBOS = list(itertools.product((1.0, 64.0), (0.0, 0.9, 1.0), (1, 23, 24, 25, 211), (-17, 0, 24, 1000))) * 8
UNSTABLE_RADIUS = 1.01
RECORDING_N = 2410
CLAMP_KINDS = ("tables", "tables_pre1", "wide")
# -p 1 takes the tables' output at -g 1000 to 3e8 only: two decades more, so that this instantiation passes int32 too
CLAMP_GAINS_PRE1 = (1, 10, 1000, 100000)
RECORDING_OPTS = dict(hop_s=0.005, n_formants=0)


@functools.lru_cache(maxsize=None)
def hostile_flows(n=HOSTILE_N):
    """(names, int16 [17][n]) of the bank; read-only"""
    names, m = hs.matrix(hs.bank(HOSTILE_FS, n, 0))
    m.setflags(write=False)
    return names, m


def saturated(pcm):
    """bool: the samples at the clamp"""
    return np.abs(pcm.astype(np.int32)) == 32767


class Case(dict):
    """the inputs of one comparison and what the restatement makes of them: flow, coefs, rows, mode, gains,
    want = (pcm, stat), state_max, lo / hi (tr.filter_track's extremes, per row)"""
    __getattr__ = dict.__getitem__


def restated(flow, coefs, rows, mode, gains=None, out=None, arith="exact"):
    peak, ext = [], []
    want = tr.filter_track(flow, coefs, rows, mode, gains, out=out, state_max=peak, extremes=ext, arith=arith)
    for a in want:
        a.setflags(write=False)
    return Case(flow=flow, coefs=coefs, rows=rows, mode=mode, gains=gains, want=want, state_max=peak[0], lo=ext[0][0],
                hi=ext[0][1])


@functools.lru_cache(maxsize=None)
def saturation_case(order, mode, with_gains):
    """reflection-drawn sets (hs.reflection_sets) on the bank's flows, every combination of SAT_COMBOS"""
    R = len(SAT_COMBOS)
    rng = np.random.default_rng(1000 + order)
    coefs = hs.reflection_sets(rng, R, SAT_K, order)
    gains = rng.uniform(0.25, 2.0, (R, SAT_K))
    combos = np.array(SAT_COMBOS)
    rows = _rows(R, SAT_K, combos[:, 2], combos[:, 3], HOSTILE_N, combos[:, 0], combos[:, 1])
    flow = hostile_flows()[1][(np.arange(R) * 7 + order) % 17]
    return restated(flow, coefs, rows, mode, gains if with_gains else None)


def check_saturation_conditions(order, mode):
    """the conditions of one (order, mode), over the calls with and without per-set gains; returns the line for the
    profile"""
    cases = [saturation_case(order, mode, g) for g in (False, True)]
    loud = cases[0].rows["gain"] == 64.0
    sat = np.concatenate([saturated(c.want[0]).ravel() for c in cases])
    lo = min(float(c.lo[loud].min()) for c in cases)
    hi = max(float(c.hi[loud].max()) for c in cases)
    for c in cases:
        assert c.state_max < STATE_FINITE
        assert not c.want[1]["status"].any() and not c.want[1]["n_unusable"].any()
        if order >= 12:                          # past int32 in both signs, in each call
            assert c.lo[loud].min() < -INT32 and c.hi[loud].max() > INT32, (order, mode, c.lo.min(), c.hi.max())
    assert 0.02 <= sat.mean() <= 0.98, sat.mean()
    return "order %2d %-5s saturated %5.1f %% (gain 1: %5.1f %%, gain 64: %5.1f %%)  o in [%.3e, %.3e]  max |y| %.3e" % (
        order, "hold" if mode == tr.HOLD else "glide", 100 * sat.mean(),
        100 * np.mean([saturated(c.want[0])[~loud].mean() for c in cases]),
        100 * np.mean([saturated(c.want[0])[loud].mean() for c in cases]), lo, hi, max(c.state_max for c in cases))


@pytest.mark.parametrize("order", SAT_ORDERS)
def test_saturation_cases_pass_int32_in_both_signs(order):
    for mode in (tr.HOLD, tr.GLIDE):
        print(check_saturation_conditions(order, mode))


def table_lanes(gains=(1, 10, 1000), pre1=False):
    """a table lane per (-g, table, bank flow): 170 lanes per gain.  The pre-emphases take turns at -g 1 and 10; at
    -g 1000 it is 0 throughout (the first difference takes a decade off the output: with -p 0 table '5' passes 2^31 on
    two flows).  pre1: -p 1 in every lane, which selects the fused kernels' instantiation for that case."""
    lanes = []
    for g in gains:
        for t, v in enumerate(TABLES):
            for r in range(17):
                p = "1" if pre1 else "0" if g >= 1000 else ["1", "0", "0.37", "0.9"][(t + r) % 4]
                lanes.append(vs.lane_from_cli(["-r", "16000", "-d", "1"], ["-v", v, "-g", "%g" % g, "-p", p], r)[0])
    return lanes


def wide_lanes(gains=(1, 10, 1000)):
    """configs.wide_order_lanes (one lane above 22 taps sends the whole batch to the wide kernel) at the same gains"""
    orders = [[1, 2, 5, 21, 22, 23, 24, 30, 31, 39, 40][i % 11] for i in range(17 * len(gains))]
    lanes, _, _ = configs.wide_order_lanes(orders)
    for i, lane in enumerate(lanes):
        lane.gain = float(gains[i // 17])
    return lanes


def lane_sets(lanes):
    """coefs [lanes][1][41] of table and custom lanes (zeros in the missing taps: they change nothing in a finite state)"""
    A = np.zeros((len(lanes), 1, 41))
    for i, l in enumerate(lanes):
        a = np.array(l.A[:]) if l.vowel == 0 else vs.vowel_coefficients(chr(l.vowel))
        A[i, 0, :len(a)] = a
    A[:, 0, 0] = 1.0
    return A


@functools.lru_cache(maxsize=None)
def clamp_case(kind, arith="exact"):
    """vs_filter's lanes as a hold track with one set: the restatement of what the oracle's filter computes, with the
    unclamped values the oracle does not show"""
    lanes = {"tables": table_lanes, "tables_pre1": lambda: table_lanes(CLAMP_GAINS_PRE1, True), "wide": wide_lanes}[kind]()
    flow = np.tile(hostile_flows()[1], (len(lanes) // 17, 1))
    rows = _rows(len(lanes), 1, 1, 0, HOSTILE_N, [l.gain for l in lanes], [l.pre_emphasis for l in lanes])
    c = restated(flow, lane_sets(lanes), rows, tr.HOLD, arith=arith)
    c["lanes"] = lanes
    return c


@pytest.mark.parametrize("kind", CLAMP_KINDS)
def test_filter_clamp_cases_pass_int32(kind):
    c = clamp_case(kind)
    assert np.array_equal(c.want[0], pyoracle.filter(c.lanes, c.flow))
    assert c.state_max < STATE_FINITE
    assert c.lo.min() < -INT32 and c.hi.max() > INT32, (c.lo.min(), c.hi.max())
    sat = saturated(c.want[0])
    print("vs_filter %-11s saturated %5.1f %%  o in [%.3e, %.3e]" % (kind, 100 * sat.mean(), c.lo.min(), c.hi.max()))
    assert 0.02 <= sat.mean() <= 0.98


@functools.lru_cache(maxsize=None)
def unstable_sets():
    """the ten tables with every root radius scaled so that the largest is UNSTABLE_RADIUS"""
    out = []
    for v in TABLES:
        A = vs.vowel_coefficients(v)
        out.append(hs.scaled_radius(A, UNSTABLE_RADIUS / _max_radius(A)))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def unstable_case(mode):
    """34 rows (the bank twice) of three unstable sets each, 400 samples per set; the second half ends early"""
    R = 34
    U = unstable_sets()
    coefs = U[(np.arange(R)[:, None] + np.array([0, 3, 7])[None, :]) % 10]
    rows = _rows(R, 3, 400, 5, np.where(np.arange(R) < 17, HOSTILE_N, HOSTILE_N - 13 * np.arange(R)), 1.0,
                 np.array([0.0, 0.9, 1.0])[np.arange(R) % 3])
    flow = np.tile(hostile_flows()[1], (2, 1))
    return restated(flow, coefs, rows, mode, out=np.full((R, HOSTILE_N), 0x5A5A, dtype=np.int16))


def test_unstable_sets_run_in_hold_mode_and_are_refused_in_glide_mode():
    for A in unstable_sets():
        assert abs(_max_radius(A) - UNSTABLE_RADIUS) < 1e-9
    hold, glide = unstable_case(tr.HOLD), unstable_case(tr.GLIDE)
    # growth is at most 1.01^1210 = 1.7e5 times what a table's own resonances make of a full-scale flow
    assert hold.state_max < STATE_FINITE and hold.state_max > 1e3 * 32768
    assert not hold.want[1]["status"].any() and not hold.want[1]["n_unusable"].any()
    assert saturated(hold.want[0]).mean() > 0.02
    assert (glide.want[1]["status"] == tr.NO_SET).all() and (glide.want[1]["n_unusable"] == 3).all()
    for r in range(34):
        n = glide.rows["length"][r]
        assert not glide.want[0][r, :n].any() and (glide.want[0][r, n:] == 0x5A5A).all()
        assert (hold.want[0][r, n:] == 0x5A5A).all()
    print("unstable hold: max |y| %.3e, saturated %.1f %%" % (hold.state_max, 100 * saturated(hold.want[0]).mean()))


@functools.lru_cache(maxsize=None)
def recording_inputs():
    """(model names, models int16 [21][n], flows int16 [21][n]): hs.track_models and, for each, another row of the bank
    as its flow; only the model `zeros` gets the silent flow"""
    names, models = hs.matrix(hs.track_models(HOSTILE_FS, RECORDING_N, 0))
    bank_names, bank = hostile_flows(RECORDING_N)
    loud = [i for i, k in enumerate(bank_names) if k != "zeros"]
    pick = []
    for i, k in enumerate(names):
        j = bank_names.index("zeros") if k == "zeros" else loud[(i + 5) % len(loud)]
        assert k == "zeros" or bank_names[j] != k
        pick.append(j)
    return names, models, bank[pick]


@functools.lru_cache(maxsize=None)
def recording_case(order, mode):
    """the sets of the LPC restatement (tests/lpc_ref.py: bit for bit the device's) on the models, 25 ms / 5 ms"""
    names, models, flow = recording_inputs()
    o = lr.opts(order=order, **RECORDING_OPTS)
    L, H, starts = lr.frame_plan(HOSTILE_FS, RECORDING_N, o)
    coefs = lr.analyse(models, HOSTILE_FS, order=order, **RECORDING_OPTS)["coefs"]
    row = tr.from_lpc(L, H, o["pre_emphasis"], len(starts), RECORDING_N, mode)
    return restated(flow, coefs, np.array([row] * len(names), dtype=tr.ROW_DTYPE), mode)


def check_recording_conditions(c):
    """the conditions of one recording case; returns the line for the profile"""
    names = recording_inputs()[0]
    nan_frames = np.isnan(c.coefs[:, :, 1:]).any(axis=2).sum(axis=1)
    assert np.array_equal(c.want[1]["n_unusable"], nan_frames)
    silent = names.index("zeros")
    assert [r for r in range(len(names)) if c.want[1]["status"][r]] == [silent] and nan_frames[silent] == c.coefs.shape[1]
    for k in ("noise_zeros", "zeros_noise", "noise_zeros_noise", "constant_zeros"):
        assert 0 < nan_frames[names.index(k)] < c.coefs.shape[1], k
    assert np.isnan(c.coefs[names.index("zeros_noise"), 0, 1]) and np.isnan(c.coefs[names.index("noise_zeros"), -1, 1])
    mid = np.isnan(c.coefs[names.index("noise_zeros_noise"), :, 1])
    assert not mid[0] and not mid[-1] and mid.any()
    assert c.state_max < STATE_FINITE
    share = saturated(c.want[0]).mean(axis=1)
    assert 3 * (share > 0.5).sum() >= len(names) and 4 * (share < 0.1).sum() >= len(names), share
    return "%d rows over 50 %% saturated, %d under 10 %%, of %d; o in [%.3e, %.3e]; max |y| %.3e; NaN frames %d" % (
        (share > 0.5).sum(), (share < 0.1).sum(), len(names), c.lo.min(), c.hi.max(), c.state_max, nan_frames.sum())


@pytest.mark.parametrize("order", [12, 22, 40])
def test_recording_cases_saturate_some_rows_and_spare_others(order):
    for mode in (tr.HOLD, tr.GLIDE):
        print("order %d %s: %s" % (order, "hold" if mode == tr.HOLD else "glide",
                                   check_recording_conditions(recording_case(order, mode))))
