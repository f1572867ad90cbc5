"""The numpy restatement of the IAIF analysis (tests/iaif_ref.py, include/voice_synth.h "IAIF") on the CPU: its fma
against libm's; the restatement against a slow scalar transcription of the header, bit for bit; stage 1 against the exact
autocorrelation of the LPC analysis; the status of every frame of the oracle's vowels and of the hostile signals; what
the feature is for -- on the residual of IAIF's sets the acoustic measure reads the shimmer of the flow more closely
than on the residual of vs_lpc's; and the host helpers of the C ABI.  The GPU tests compare the device with this
restatement, which carries these checks over."""
import ctypes as C
import functools
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
import hostile_signals as hs  # noqa: E402
import iaif_ref as ia  # noqa: E402
import inverse_ref as ir  # noqa: E402
import lpc_ref as lr  # noqa: E402
import track_ref as tr  # noqa: E402
from test_acoustic_ref import speech  # noqa: E402

_libm_fma = tr._libm.fma


# 1 ---- consistency of the restatement

def test_the_vectorised_fma_is_libms():
    rng = np.random.default_rng(0)
    n = 200000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    c = -(a * b) * (1.0 + rng.integers(-4, 5, n) * 2.0 ** -52)        # a*b + c cancels to the last bits
    c[::3] = rng.standard_normal(len(c[::3])) * 10.0 ** rng.integers(-8, 9, len(c[::3]))
    c[::7] = 0.0
    a[::11] = np.rint(a[::11])                                        # integers: exact products, ties
    b[::11] = np.rint(b[::11]) + 0.5
    want = tr.fma(a, b, c)
    assert np.array_equal(ia.fma(a, b, c), want)
    assert (want != a * b + c).sum() > n // 10                        # (the two roundings differ: something is tested)
    z = np.zeros(4)
    assert np.array_equal(ia.fma(z, [1.0, -2.0, 0.0, 5.0], z), z) and not np.signbit(ia.fma(z, [1.0, -2.0, 0.0, 5.0], z)).any()


def scalar_iaif(x, s, L, w, p, g, rho):
    """the header's section, transcribed sample by sample on Python floats with libm's fma: (r0, err, status, V2, c2)"""
    M = p + 1
    nan = math.nan

    def e(n):                                    # the extended frame
        return float(x[s + n]) if n >= -M and s + n >= 0 else 0.0

    def fir(c):
        y = {}
        for n in range(-M, L):
            acc = e(n)
            for j in range(1, len(c) + 1):
                acc = _libm_fma(c[j - 1], e(n - j) if n - j >= -M else 0.0, acc)
            y[n] = acc
        return y

    def integ(y):
        out, prev = {}, 0.0
        for n in range(-M, L):
            prev = _libm_fma(rho, prev, y[n])
            out[n] = prev
        return out

    def lpc(y, q):
        v = [float(w[n]) * y[n] for n in range(L)]
        r = []
        for k in range(q + 1):
            acc = 0.0
            for n in range(L - k):
                acc = _libm_fma(v[n], v[n + k], acc)
            r.append(acc)
        A, err, st = lr.levinson(r, q)
        return r[0], A, err, st

    c2 = [1.0] + [nan] * g
    taps = []
    for stage, q in ((1, 1), (2, p), (3, g), (4, p)):
        y = fir(taps)
        if stage == 3:
            y = integ(y)
        r0, A, err, st = lpc(y, q)
        if st:
            return r0, nan, st, [1.0] + [nan] * p, c2
        taps = A[1:]
        if stage == 3:
            c2 = A
    return r0, err, 0, A, c2


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("kw", [dict(order=22, glottal_order=4, hop_s=0.0125),
                                dict(order=22, glottal_order=9, leak=1.0, hop_s=0.001, window="rectangular"),
                                dict(order=1, glottal_order=1, leak=0.0, hop_s=0.02)])
def test_the_restatement_is_the_scalar_transcription_bit_for_bit(kw):
    """a vowel, noise, a tone in noise and a row of zeros then a pulse (silent frames, and frames that end at a later
    stage); frames at s = 0, at 0 < s < M (hop 1 ms) and further in"""
    fs, n = 16000, 900
    lane = vs.lane_from_cli(["-r", "16000", "-d", "1", "-f", "110", "-s", "5"], ["-v", "a"], 3)[0]
    bank = hs.bank(fs, n, 1)
    x = np.stack([pyoracle.synth([lane], n)[0], bank["noise_full"], bank["sine_150_noise"], bank["impulses_110"]])
    x[3, :500] = 0
    if kw["hop_s"] == 0.001:
        x = x[:, :440]
    res = ia.analyse(x, fs, **kw)
    o = ia.opts(**kw)
    L, H, starts = lr.frame_plan(fs, x.shape[1], ia.lpc_opts(o))
    w = lr.window(L, o["window"])
    picked = sorted({0, 1, len(starts) - 1})
    seen = set()
    for i in range(x.shape[0]):
        for j in picked:
            r0, err, st, A, c2 = scalar_iaif(x[i], starts[j], L, w, o["order"], o["glottal_order"], o["leak"])
            seen.add(st)
            assert res["status"][i, j] == st and res["start"][i, j] == starts[j], (i, j)
            assert _same(res["r0"][i, j], r0) and _same(res["err"][i, j], err), (i, j)
            assert _same(res["coefs"][i, j], A) and _same(res["glottal"][i, j], c2), (i, j)
    assert 0 in seen and lr.SILENT in seen


def test_stage_one_is_the_exact_autocorrelation():
    """|x| <= 1000 and L = 400: every sum of v[n] v[n+k] stays below 400 * (256 * 1000)^2 = 2.6e13 < 2^53, so the fma
    chain is exact and must equal the int64 dot product of lpc_ref"""
    rng = np.random.default_rng(4)
    fs, n = 16000, 2000
    x = rng.integers(-1000, 1001, (3, n)).astype(np.int16)
    res = ia.analyse(x, fs, order=6, glottal_order=2)
    L, H, starts = lr.frame_plan(fs, n, lr.opts(order=6))
    w = lr.window(L)
    for i in range(3):
        for j, s in enumerate(starts):
            want = [float(t) for t in lr.autocorr(x[i], s, L, 1, w, 0)]
            assert list(res["r_stage1"][i, j]) == want and abs(want[0]) < 2.0 ** 53


# 2 ---- status

def test_hostile_signals_status_and_taps():
    fs, n = 16000, 4000
    names, pcm = hs.matrix(hs.bank(fs, n, 0))
    for p, g in ((22, 4), (40, 6)):
        res = ia.analyse(pcm, fs, order=p, glottal_order=g)
        st = res["status"]
        for i, name in enumerate(names):
            print("order %2d %-15s frames with status 0 / SILENT / UNSTABLE: %d / %d / %d" % (
                p, name, (st[i] == 0).sum(), (st[i] == lr.SILENT).sum(), (st[i] == lr.UNSTABLE).sum()))
        assert (st[names.index("zeros")] == lr.SILENT).all() and (res["r0"][names.index("zeros")] == 0.0).all()
        bad = st != 0
        assert np.isnan(res["coefs"][bad][:, 1:]).all() and np.isnan(res["err"][bad]).all()
        assert np.isnan(res["glottal"][bad][:, 1:]).all()      # (none of these frames ends as late as stage 4)
        assert np.isfinite(res["coefs"][~bad]).all() and np.isfinite(res["glottal"][~bad]).all()
        assert np.isfinite(res["err"][~bad]).all() and (res["coefs"][..., 0] == 1.0).all()


# 3 ---- what the feature is for

@functools.lru_cache(maxsize=None)
def shimmer_table(S, de_emphases=(0.99,)):
    """the 16 oracle vowels of tests/test_inverse_ref.py at set shimmer S %: the mean local shimmer on the flow and,
    per (de-emphasis, polarity), on the residual with vs_lpc's sets and with IAIF's sets (hold, scale 1/10).  Returns
    (on_flow, {(rho, polarity): (lpc, iaif)}, all frames of IAIF at status 0)"""
    lanes, ns, pcm = speech(["-s", str(S)], [], 300, n=16)
    flow = pyoracle.source(lanes, ns)
    fs = 22050
    sets = {"lpc": lr.analyse(pcm, fs)["coefs"], "iaif": ia.analyse(pcm, fs)}
    ok = bool((sets["iaif"]["status"] == 0).all())
    sets["iaif"] = sets["iaif"]["coefs"]
    L, H, starts = lr.frame_plan(fs, ns, lr.opts())
    n_sets, hop, offset, length = ir.from_lpc(L, H, 0, len(starts), ns, ir.HOLD)[:4]
    on_flow = float(ar.measure(flow, fs)["shimmer_local"].mean())
    table = {}
    for rho in de_emphases:
        rows = ir.rows_of(16, n_sets, hop, offset, ns, 1.0 / lanes[0].gain, rho)
        inv = {k: ir.inverse_filter(pcm, sets[k], rows, ir.HOLD)[0] for k in sets}
        for pol in (1, -1):
            table[(rho, pol)] = tuple(float(ar.measure(inv[k], fs, polarity=pol)["shimmer_local"].mean())
                                      for k in ("lpc", "iaif"))
    return on_flow, table, ok


# the gaps |IAIF - flow| at polarity +1, de-emphasis 0.99, as this test printed them (S = 2, 5, 10), and their bound
PRINTED_GAPS = {2: 0.0007, 5: 0.0016, 10: 0.0019}
GAP_BOUND = 2 * max(PRINTED_GAPS.values())


@pytest.mark.parametrize("S", [2, 5, 10])
def test_iaif_sets_read_the_shimmer_of_the_flow_more_closely_than_lpc_sets(S):
    """order 22, 25 ms Hamming, hop 10 ms, glottal order 4, leak 0.99; inverse: hold, scale 1/10, de-emphasis 0.99;
    measured at polarity +1.  Printed by this test (mean local shimmer of 16 rows):

        S     on the flow   LPC sets   IAIF sets   |LPC - flow|   |IAIF - flow|   polarity -1: LPC sets, IAIF sets
        2       0.0203       0.0262     0.0196       0.0059          0.0007            0.0301    0.0323
        5       0.0503       0.0430     0.0488       0.0074          0.0016            0.0547    0.0747
        10      0.1017       0.0755     0.0997       0.0262          0.0019            0.1030    0.1566

    Asserted: every frame at status 0; IAIF closer to the flow than LPC for each S; the gap within twice the largest
    printed one.  Polarity -1, where IAIF does worse than LPC, is printed only."""
    on_flow, table, ok = shimmer_table(S)
    lpc, iaif = table[(0.99, 1)]
    print("set shimmer %2d %%: on the flow %.4f, residual with vs_lpc sets %.4f, with IAIF sets %.4f: gaps %.4f and %.4f; "
          "polarity -1: %.4f and %.4f" % ((S, on_flow, lpc, iaif, abs(lpc - on_flow), abs(iaif - on_flow))
                                          + table[(0.99, -1)]))
    assert ok
    assert abs(iaif - on_flow) < abs(lpc - on_flow)
    assert abs(iaif - on_flow) <= GAP_BOUND


# 4 ---- the host helpers of the C ABI (no device)

def test_defaults_and_the_lpc_options_of_the_same_frames():
    lib = vs.load()
    o = _ffi.IaifOpts()
    assert C.sizeof(_ffi.IaifOpts) == 56
    assert lib.vs_iaif_defaults(None) == _ffi.VS_ERR_ARG and lib.vs_iaif_defaults(C.byref(o)) == 0
    assert (o.order, o.glottal_order, o.window, o.n_formants, o.reserved_) == (22, 4, vs.VS_LPC_HAMMING, 5, 0)
    assert (o.window_s, o.hop_s, o.f_lo, o.leak) == (0.025, 0.010, 50.0, 0.99)
    lo = _ffi.LpcOpts()
    assert lib.vs_iaif_lpc_opts(C.byref(o), None) == _ffi.VS_ERR_ARG
    for opts in (None, C.byref(o)):
        assert lib.vs_iaif_lpc_opts(opts, C.byref(lo)) == 0
        assert (lo.order, lo.window, lo.pre_emphasis, lo.n_formants, lo.reserved_) == (22, vs.VS_LPC_HAMMING, 0, 5, 0)
        assert (lo.window_s, lo.hop_s, lo.f_lo) == (0.025, 0.010, 50.0)
    kw = dict(order=18, glottal_order=6, window="rectangular", window_s=0.03, hop_s=0.0, n_formants=7, f_lo=80.0, leak=0.5)
    got = vs.iaif_lpc_opts(**kw)
    assert got == dict(order=18, window=vs.VS_LPC_RECTANGULAR, window_s=0.03, hop_s=0.0, pre_emphasis=0, n_formants=7,
                       f_lo=80.0)
    # the frame plan: vs_lpc_frames and the rows of the tracks and the inverse, unchanged
    assert vs.lpc_frames(16000, 16000, **vs.iaif_lpc_opts()) == 98
    assert tuple(vs.inverse_from_lpc(16000, 16000, "hold", **vs.iaif_lpc_opts())) == (98, 160, 120, 16000, 1.0, 0.0)
    assert tuple(vs.track_from_lpc(16000, 16000, "glide", **vs.iaif_lpc_opts()))[:4] == (98, 160, 200, 16000)


def test_refusals():
    lib = vs.load()
    lo = _ffi.LpcOpts()

    def rc(**kw):
        reserved = kw.pop("reserved_", 0)
        o = vs.iaif_opts(**kw)
        o.reserved_ = reserved
        return lib.vs_iaif_lpc_opts(C.byref(o), C.byref(lo))

    assert rc() == 0 and rc(glottal_order=22) == 0 and rc(order=40, glottal_order=40) == 0
    assert rc(leak=0.0) == 0 and rc(leak=1.0) == 0 and rc(order=1, glottal_order=1) == 0
    for kw in (dict(glottal_order=0), dict(glottal_order=23), dict(order=4, glottal_order=5), dict(glottal_order=-1),
               dict(leak=-1e-9), dict(leak=1.0000001), dict(leak=math.nan), dict(leak=math.inf), dict(order=0),
               dict(order=41)):
        assert rc(**kw) == _ffi.VS_ERR_RANGE, kw
    for kw in (dict(reserved_=1), dict(window=5), dict(n_formants=21), dict(n_formants=-1), dict(f_lo=-1.0),
               dict(hop_s=-0.01), dict(window_s=math.nan)):
        assert rc(**kw) == _ffi.VS_ERR_ARG, kw
    # the launch refuses the same before it touches a device: no context, no buffers
    o = vs.iaif_opts()
    assert lib.vs_iaif_launch(None, C.byref(o), None, 0, 0, 0, None, None, 0, None, None, None, None) == _ffi.VS_ERR_ARG
    assert lib.vs_iaif(None, C.byref(o), None, 0, 0, 0, None, None, 0, None, None, None, None) == _ffi.VS_ERR_ARG
