"""The glottal parameters without a device: the records' ABI, the options and the errors vs_glottal_launch answers before
it touches the device, and the numpy restatement (tests/glottal_ref.py) of include/voice_synth.h, "glottal parameters",
held to what the CPU oracle's pulses are made of, to what the feature is for, and to signals nobody synthesises."""
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
import acoustic_ref as ar  # noqa: E402
import glottal_ref as gr  # noqa: E402
import hostile_signals as hs  # noqa: E402
import inverse_ref as ir  # noqa: E402
from test_acoustic_ref import speech  # noqa: E402

LEVELS = ((0, 128), (26, 128), (255, 255))


# 1 ---- ABI, defaults, errors

def test_record_sizes():
    assert C.sizeof(_ffi.GlottalOpts) == gr.OPTS_DTYPE.itemsize == 16
    assert C.sizeof(_ffi.GlottalRec) == vs.GLOTTAL_DTYPE.itemsize == gr.REC_DTYPE.itemsize == 56
    assert C.sizeof(_ffi.GlottalCycle) == vs.GLOTTAL_CYCLE_DTYPE.itemsize == gr.CYCLE_DTYPE.itemsize == 48
    assert vs.GLOTTAL_DTYPE == gr.REC_DTYPE and vs.GLOTTAL_CYCLE_DTYPE == gr.CYCLE_DTYPE
    assert [f[0] for f in _ffi.GlottalRec._fields_] == list(gr.REC_DTYPE.names)
    assert [f[0] for f in _ffi.GlottalCycle._fields_] == list(gr.CYCLE_FIELDS)
    assert (gr.GL_NO_CYCLES, gr.GL_BAD_MARKS, gr.GL_REJECTED, gr.GL_ALL_REJECTED) == (
        vs.VS_GL_NO_CYCLES, vs.VS_GL_BAD_MARKS, vs.VS_GL_REJECTED, vs.VS_GL_ALL_REJECTED)
    assert (gr.GLC_ZERO_AMPLITUDE, gr.GLC_NO_CLOSURE) == (vs.VS_GLC_ZERO_AMPLITUDE, vs.VS_GLC_NO_CLOSURE)


def test_defaults():
    o = vs.glottal_opts()
    assert (o.level_open, o.level_mid, o.polarity, o.reserved_) == (26, 128, 1, 0)
    assert vs.load().vs_glottal_defaults(None) == _ffi.VS_ERR_ARG


def _launch(opts=None, ctx=True, pcm=True, pitch=100, n_lanes=2, n_samples=100, meas=True, marks=True, marks_pitch=8,
            out=True, cycles=False, cycles_pitch=0):
    """vs_glottal_launch with pointers that are never followed: every case below is answered from the arguments alone"""
    block = (C.c_char * 4096)()
    p = C.addressof(block)
    return vs.load().vs_glottal_launch(p if ctx else None, C.byref(opts) if opts is not None else None, p if pcm else None,
                                       pitch, n_lanes, n_samples, p if meas else None, p if marks else None, marks_pitch,
                                       p if out else None, p if cycles else None, cycles_pitch)


def test_launch_errors_that_need_no_device():
    for what in ("ctx", "pcm", "meas", "marks", "out"):
        assert _launch(**{what: False}) == _ffi.VS_ERR_ARG, what
    assert _launch(n_lanes=0) == _launch(n_samples=0) == _launch(marks_pitch=0) == _ffi.VS_ERR_ARG
    assert _launch(pitch=99) == _ffi.VS_ERR_ARG
    assert _launch(cycles=True, cycles_pitch=0) == _ffi.VS_ERR_ARG
    assert _launch(n_lanes=1 << 31) == _ffi.VS_ERR_UNSUPPORTED
    assert _launch(n_samples=1 << 31, pitch=1 << 31) == _ffi.VS_ERR_UNSUPPORTED
    assert _launch(marks_pitch=1 << 31) == _ffi.VS_ERR_UNSUPPORTED
    assert _launch(cycles=True, cycles_pitch=1 << 31) == _ffi.VS_ERR_UNSUPPORTED
    for lo, mid in ((-1, 128), (256, 256), (26, 25), (26, 256)):
        assert _launch(vs.glottal_opts(lo, mid)) == _ffi.VS_ERR_RANGE, (lo, mid)
    for pol in (0, 2, -2):
        assert _launch(vs.glottal_opts(polarity=pol)) == _ffi.VS_ERR_ARG
    o = vs.glottal_opts()
    o.reserved_ = 1
    assert _launch(o) == _ffi.VS_ERR_ARG
    for bad in ((-1, 128, 1), (26, 25, 1), (26, 128, 0)):
        with pytest.raises(ValueError):
            gr.check_levels(*bad)


# 2 ---- level 0 on the CPU oracle's clean flows

def _t2(lane):
    P = int(np.float32(lane.fs) / np.float32(lane.F0))                      # fg:244
    return int(math.ceil(0.5 * float(np.float32(lane.cq)) * P))             # fg:317


@pytest.mark.parametrize("args", [[], ["-j", "2", "-s", "5"]])
def test_level_zero_reads_the_pulse_the_oracle_made(args):
    """F0 100, fs 22050, 1 s: rise = T2 - 1 in every cycle, one fall per row, the period is the logged T"""
    for seed in (0, 7):
        lane, d = vs.lane_from_cli(["-d", "1", "-f", "100"] + args, ["-v", "a"], seed)
        n = vs.num_samples(22050, d)
        flow, recs, ncyc, _ = pyoracle.source_one(lane, n, 400)
        _, _, rec, cyc = gr.measure_and_glottal(flow[None, :], 22050, level_open=0, cycles_pitch=200)
        nc = int(rec["n_cycles"][0])
        c = cyc[0, :nc]
        assert rec["status"][0] == 0 and rec["n_rejected"][0] == 0 and nc >= 60
        assert not c["status"].any()
        assert np.all(c["peak"] - c["open"] == _t2(lane) - 1), (np.unique(c["peak"] - c["open"]), _t2(lane))
        assert len(np.unique(c["close"] - c["peak"])) == 1
        # the logged cycle each peak lies in (with shimmer the first mark may be the second cycle's peak)
        starts = np.concatenate([[0], np.cumsum(recs["T"][:ncyc])])
        k = np.searchsorted(starts, c["peak"], side="right") - 1
        assert np.array_equal(np.diff(k), np.ones(nc - 1, dtype=k.dtype))
        assert np.array_equal(c["period"], recs["T"][k])
        assert np.array_equal(c["open"], starts[k] + 1)
        if not args and seed == 0:
            assert (_t2(lane) - 1, int(c["close"][0] - c["peak"][0])) == (60, 42)


# 3 ---- what it is for: the pulse shape read from inverse-filtered speech

@pytest.fixture(scope="module", params=[[], ["-s", "5", "-j", "2"], ["-s", "10"]], ids=["plain", "s5j2", "s10"])
def three_signals(request):
    """16 of the CPU oracle's vowels of tests/test_acoustic_ref.py (seeds 300.., -v a, gain 10, pre-emphasis 1), their
    flows, and the speech inverse-filtered with the known table as in tests/test_inverse_ref.py; measured once"""
    lanes, ns, pcm = speech(request.param, [], 300, n=16)
    flow = pyoracle.source(lanes, ns)
    coefs = np.broadcast_to(vs.vowel_coefficients("a"), (16, 1, 23))
    inv, stat = ir.inverse_filter(pcm, coefs, ir.rows_of(16, 1, 1, 0, ns, 1.0 / lanes[0].gain, lanes[0].pre_emphasis),
                                  ir.HOLD)
    assert not stat["status"].any()
    sig = {}
    for name, x in (("flow", flow), ("inverse", inv), ("speech", pcm)):
        meas, marks = ar.measure(x, 22050, marks=ns // 2 + 2)
        sig[name] = (x, meas, marks)
    return request.param, sig


@pytest.mark.parametrize("level_open", [13, 26])
def test_inverse_filtered_vowels_read_the_pulse_shape_of_the_flow(three_signals, level_open):
    """OQ, QOQ and NAQ of the known-filter inverse lie within 0.002 of the flow's (measured: at most 0.0003); the speech
    itself reads QOQ 0.05 and NAQ 0.033 whatever was set: at least 0.19 and 0.09 away (measured 0.197..0.21, 0.099..0.107)"""
    args, sig = three_signals
    mean = {}
    for name, (x, meas, marks) in sig.items():
        r = gr.glottal(x, meas, marks, level_open=level_open)
        assert np.all(r["n_cycles"] > 0)
        mean[name] = {f: float(r[f].mean()) for f in gr.FIELDS}
        print(args, level_open, name, " ".join("%s %.4f" % (f, mean[name][f]) for f in gr.FIELDS))
    for f in ("oq", "qoq", "naq"):
        assert abs(mean["inverse"][f] - mean["flow"][f]) <= 0.002, f
    assert abs(mean["speech"]["qoq"] - mean["flow"]["qoq"]) >= 0.19
    assert abs(mean["speech"]["naq"] - mean["flow"]["naq"]) >= 0.09


# 4 ---- the hostile bank

def hostile_case(case, polarity, marks_pitch=None):
    """(names, pcm, meas, marks) of one of hostile_signals.ACOUSTIC_CASES on the restatement of the measurement"""
    fs, n, f0_min, f0_max = case
    names, pcm = hs.matrix(hs.bank(fs, n))
    meas, marks = ar.measure(pcm, fs, f0_min, f0_max, polarity, marks=marks_pitch or n // 2 + 2)
    return names, pcm, meas, marks


def check_cycle_order(cyc, rec):
    """every accepted cycle: open <= open_mid <= peak < close_mid <= close < next peak, decl > 0; every rejected one: -1
    and decl 0.  Returns (accepted, rejected)"""
    acc = rej = 0
    for i in range(cyc.shape[0]):
        nc = int(rec["n_cycles"][i] + rec["n_rejected"][i])
        c = cyc[i, :nc]
        ok = c["status"] == 0
        a, r = c[ok], c[~ok]
        assert np.all((a["trough"] < a["open"]) & (a["open"] <= a["open_mid"]) & (a["open_mid"] <= a["peak"])
                      & (a["peak"] < a["close_mid"]) & (a["close_mid"] <= a["close"])
                      & (a["close"] < a["peak"] + a["period"]) & (a["decl"] > 0) & (a["amp"] > 0)
                      & (a["gci"] > a["peak"]) & (a["gci"] <= a["close"]))
        for f in ("open", "close", "open_mid", "close_mid", "gci"):
            assert np.all(r[f] == -1)
        assert np.all(r["decl"] == 0)
        assert int(ok.sum()) == rec["n_cycles"][i]
        acc += int(ok.sum())
        rej += int((~ok).sum())
    return acc, rej


def test_hostile_bank_in_the_restatement():
    acc = rej = 0
    for case in hs.ACOUSTIC_CASES:
        for polarity in (1, -1):
            names, pcm, meas, marks = hostile_case(case, polarity)
            for lo, mid in LEVELS:
                rec, cyc = gr.glottal(pcm, meas, marks, lo, mid, polarity, cycles_pitch=marks.shape[1])
                a, r = check_cycle_order(cyc, rec)
                acc += a
                rej += r
                empty = rec["n_cycles"] == 0
                assert np.all(np.isnan(rec["oq"][empty])) and not np.isnan(rec["naq"][~empty]).any()
    print("hostile bank: %d accepted and %d rejected cycles" % (acc, rej))
    assert acc > 1000 and rej > 1000


# 5 ---- fabricated marks

def fabricated_marks(n_samples, marks_pitch=8):
    """(n_periods, status, marks) rows: the first is good, the rest fail the check as a whole (or have no cycles); every
    value lies inside [-n_samples, 2*n_samples)"""
    n = n_samples
    good = [n // 8, n // 4, n // 2, n - n // 4, n - 1, -1, -1, -1]
    rows = [(4, 0, good),
            (4, 0, [n // 8, n // 2, n // 4, n - n // 4, n - 1, -1, -1, -1]),      # not increasing
            (4, 0, [n // 8, n // 4, n // 4, n - n // 4, n - 1, -1, -1, -1]),      # equal
            (4, 0, [-3, n // 4, n // 2, n - n // 4, n - 1, -1, -1, -1]),          # negative first
            (4, 0, [-n, -n // 2, -1, n - n // 4, n - 1, -1, -1, -1]),             # increasing, negative
            (4, 0, [n // 8, n // 4, n // 2, n - n // 4, n, -1, -1, -1]),          # last = n_samples
            (4, 0, [n // 8, n // 4, n // 2, n + n // 4, 2 * n - 1, -1, -1, -1]),  # beyond the row
            (-1, 0, good), (-2 ** 31, 0, good),                                   # n_periods negative
            (7, 0, good),                                                         # the marks' row ends in -1
            (100, 0, good), (2 ** 31 - 1, 0, good),                               # beyond marks_pitch: -1 is inside M
            (4, ar.AC_UNVOICED, good), (1, 0, good)]                              # no cycles
    assert all(len(m) == marks_pitch for _, _, m in rows)
    meas = np.zeros(len(rows), dtype=ar.DTYPE)
    meas["n_periods"] = [r[0] for r in rows]
    meas["status"] = [r[1] for r in rows]
    return meas, np.array([r[2] for r in rows], dtype=np.int32)


def test_fabricated_marks_in_the_restatement():
    n = 600
    rng = np.random.default_rng(5)
    pcm = rng.integers(-3000, 3000, size=(14, n)).astype(np.int16)
    meas, marks = fabricated_marks(n)
    rec, cyc = gr.glottal(pcm, meas, marks, cycles_pitch=4)
    assert rec["status"][0] & ~gr.GL_REJECTED == 0 and rec["n_cycles"][0] + rec["n_rejected"][0] == 3
    assert np.all(rec["status"][1:12] == gr.GL_BAD_MARKS)
    assert np.all(rec["status"][12:] == gr.GL_NO_CYCLES)
    assert np.all(rec["n_cycles"][1:] == 0) and np.all(rec["n_rejected"][1:] == 0) and np.isnan(rec["oq"][1:]).all()
    assert cyc[1:].tobytes() == b"\xff" * (13 * 4 * 48) and np.all(cyc[0, 3]["peak"] == -1)
    # n_periods beyond marks_pitch with marks that fill the row: the first marks_pitch marks are measured
    meas2 = meas[:1].copy()
    meas2["n_periods"] = 100
    rec2, cyc2 = gr.glottal(pcm[:1], meas2, marks[:1, :5], cycles_pitch=4)
    assert rec2.tobytes() == rec[:1].tobytes() and cyc2.tobytes() == cyc[:1].tobytes()


def test_format_line():
    rec = dict(oq=0.39551, clq=0.17, sq=1.230769, qoq=0.2545, naq=float("nan"), n_cycles=98, n_rejected=1, status=4)
    assert gr.format_line("a.wav", rec) == "a.wav 0.3955 0.1700 1.2308 0.2545 nan 98 1 4"
