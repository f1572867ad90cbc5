"""The numpy restatement of the closed-phase covariance LPC (tests/cplpc_ref.py, include/voice_synth.h "closed-phase
covariance LPC") on the CPU: the exact recurrence of the covariance against the direct sum; a synthetic free response;
every status path; the acceptance rule at its edges; the frames; what the feature is for -- blind, the closed-phase sets
read shimmer, OQ, QOQ and NAQ of the flow where IAIF's do not; and the host helpers of the C ABI.  The GPU tests compare
the device with this restatement, which carries these checks over."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import cplpc_ref as cp  # noqa: E402
import glottal_ref as gl  # noqa: E402
import lpc_ref as lr  # noqa: E402
import track_ref as tr  # noqa: E402


def records(spans, rows=1, cycles_pitch=None):
    """hand-built records for one row: a cycle per span (b, e) with close = b - 4 and period = e - b, to be read with
    delay 4 and span_q 256"""
    cpitch = len(spans) if cycles_pitch is None else cycles_pitch
    R = np.zeros(rows, dtype=gl.REC_DTYPE)
    Cy = np.zeros((rows, max(cpitch, 1)), dtype=gl.CYCLE_DTYPE)
    R["n_cycles"] = len(spans)
    for c, (b, e) in enumerate(spans[:cpitch]):
        Cy["close"][:, c] = b - 4
        Cy["period"][:, c] = e - b
    return R, Cy


WHOLE = dict(delay=4, span_q=256)


def one(x, spans, **kw):
    """the single frame of one row x over hand-built spans: analyse()'s dict with the leading axes dropped"""
    R, Cy = records(spans)
    res = cp.analyse(np.asarray(x)[None, :], 16000, R, Cy, **dict(WHOLE, **kw))
    return {k: (v[0, 0] if isinstance(v, np.ndarray) and v.ndim >= 2 else v[0]) for k, v in res.items()}


# 1 ---- the covariance

@pytest.mark.parametrize("p", [1, 2, 22, 40])
def test_the_recurrence_is_the_direct_sum(p):
    """random int16 rows that hold the extreme values +-32766, spans of p + 1 samples and longer, overlapping ones too"""
    rng = np.random.default_rng(p)
    x = rng.integers(-32766, 32767, 3000).astype(np.int16)
    x[rng.integers(0, 3000, 300)] = rng.choice([-32766, 32766], 300)
    spans = [(0, p + 1), (7, 7 + p + 2), (100, 400), (350, 900), (2000, 3000), (2999 - p, 3000)]
    direct, rec = cp.phi_direct(x, spans, p), cp.phi_recurrence(x, spans, p)
    assert (direct == rec).all() and (direct == direct.T).all()
    assert all(isinstance(v, int) for v in direct.ravel()) and int(direct[0, 0]) > 2 ** 31
    # phi(0, 0) by hand
    assert direct[0, 0] == sum(int(v) ** 2 for b, e in spans for v in x[b + p:e])


# 2 ---- a synthetic free response

def resonator_bank(p, seed):
    """the poles of an order-p all-pole filter that rings long and evenly: p / 2 resonances a tenth of their spacing off
    an even spread over the band, radii 0.99995 .. 0.99999.  An even spread is what keeps the covariance matrix of the
    response well conditioned (printed below: under 6), so that the rounding to int16 reaches the taps undiminished but
    not amplified; the offsets make every tap non-zero (up to 0.18)."""
    rng = np.random.default_rng(seed)
    n = p // 2
    f = (np.arange(n) + 0.5 + rng.uniform(-0.1, 0.1, n)) / n * np.pi
    z = (0.99997 + rng.uniform(-0.00002, 0.00002, n)) * np.exp(1j * f)
    return np.concatenate([z, z.conj()])


def rung_once(z, n, peak):
    """(A, h): A(z) with those roots, and the first n samples of 1 / A(z)'s response to a unit impulse, h[t] = [t == 0] -
    sum_j A[j] h[t - j], scaled to the peak and rounded to int16"""
    A = np.real(np.poly(z))
    p = len(A) - 1
    h = np.zeros(n + p)                                  # h[t] at h[p + t]
    rev = A[:0:-1].copy()                                # A[p] .. A[1]
    for t in range(n):
        h[p + t] = (1.0 if t == 0 else 0.0) - float(np.dot(rev, h[t:t + p]))
    h = h[p:]
    return A, np.round(h * (peak / np.abs(h).max())).astype(np.int16)


# the largest max |a_j - A_j| and the largest err / r0 of the three orders as the test below printed them, and the bounds:
# 3 times those, which lie within the 1e-6 per tap and the 1e-7 the definition of this test names
PRINTED_FREE_RESPONSE = (7.1e-08, 2.7e-08)
TAP_BOUND, ERR_BOUND = 3 * PRINTED_FREE_RESPONSE[0], 3 * PRINTED_FREE_RESPONSE[1]
assert TAP_BOUND <= 1e-6 and ERR_BOUND <= 1e-7


@pytest.mark.parametrize("p", [2, 22, 40])
def test_a_free_response_gives_its_filter_back(p):
    """An order-p all-pole filter (resonator_bank) rung once by a unit impulse, 60000 samples scaled to a peak of 32000
    and rounded to int16; spans anywhere after the excitation: [5, 20005), [21000, 30000), [31000, 60000).  Printed by
    this test:

        order   max |a_j - A_j|   err / r0     cond(phi[1:, 1:])   largest |A_j|, 0 < j < p (order 2: |A_1|)
        2         8.2e-10         1.6e-09        1.4e+00             0.298
        22        4.4e-08         1.4e-08        5.2e+00             0.184
        40        7.1e-08         2.7e-08        3.5e+00             0.119

    Asserted at every order: status 0, every tap within TAP_BOUND = 2.1e-07 and err / r0 below ERR_BOUND = 8.1e-08 (3
    times the largest figure printed; both inside 1e-6 and 1e-7), and the solve within 1e-9 of numpy.linalg.solve on the
    same matrix.  What the bounds rest on: the rounding is noise of 0.29 LSB rms, and a response that rings for tens of
    thousands of samples under a well-conditioned covariance matrix averages it down to 1e-8 .. 1e-7 of a tap.  Sharp
    resonances crowded together do not allow that (their matrix has a condition of 1e6 and more, and the same rounding
    moves taps by units); on vowels the taps are off by 0.01 .. 0.07 and the flow is still reached (test 6)."""
    A, h = rung_once(resonator_bank(p, p), 60000, 32000.0)
    spans = [(5, 20005), (21000, 30000), (31000, 60000)]
    r = one(h, spans, order=p)
    phi = np.asarray(cp.phi_direct(h, spans, p), dtype=np.float64)
    tap = float(np.abs(r["coefs"] - A).max())
    q = float(r["err"] / r["r0"])
    print("order %2d: max |a_j - A_j| %.1e, err / r0 %.1e, cond %.1e, largest inner |A_j| %.3f, status %d" % (
        p, tap, q, np.linalg.cond(phi[1:, 1:]), np.abs(A[1:-1]).max(), r["status"]))
    assert r["status"] == 0
    assert tuple(r["counts"]) == (3, sum(e - b - p for b, e in spans))
    assert tap <= TAP_BOUND and 0 <= q <= ERR_BOUND
    assert np.abs(r["coefs"][1:] - np.linalg.solve(phi[1:, 1:], -phi[1:, 0])).max() < 1e-9


# 3 ---- every status path

def test_few_equations_at_the_threshold():
    rng = np.random.default_rng(3)
    x = rng.integers(-3000, 3000, 400).astype(np.int16)
    p = 6
    for need, kw in ((2 * p, {}), (p, dict(min_equations=p)), (31, dict(min_equations=31))):
        short = one(x, [(10, 10 + p + need - 1)], order=p, **kw)          # n_eq = need - 1
        enough = one(x, [(10, 10 + p + need)], order=p, **kw)
        assert short["status"] == cp.FEW_EQUATIONS and tuple(short["counts"]) == (1, need - 1)
        assert np.isnan(short["coefs"][1:]).all() and np.isnan(short["err"]) and short["coefs"][0] == 1.0
        assert short["r0"] == float(sum(int(v) ** 2 for v in x[10 + p:10 + p + need - 1]))
        assert enough["status"] & cp.FEW_EQUATIONS == 0 and np.isfinite(enough["coefs"]).all()
    none = one(x, [], order=p)
    assert none["status"] == cp.FEW_EQUATIONS and none["r0"] == 0.0 and tuple(none["counts"]) == (0, 0)


def test_silent_and_singular():
    z = one(np.zeros(500, np.int16), [(10, 300)], order=22)
    assert z["status"] == cp.SILENT and z["r0"] == 0.0 and np.isnan(z["coefs"][1:]).all() and np.isnan(z["err"])
    c = one(np.full(500, 1234, np.int16), [(10, 300)], order=22)
    assert c["status"] == cp.SINGULAR and c["r0"] > 0 and np.isnan(c["coefs"][1:]).all() and np.isnan(c["err"])
    t = np.arange(2000)
    tone = np.round(20000 * np.sin(2 * np.pi * t / 8.0)).astype(np.int16)  # eight exact values: rank 2
    s = one(tone, [(16, 1616)], order=22)
    assert s["status"] == cp.SINGULAR and np.isnan(s["coefs"][1:]).all()
    ok = one(tone, [(16, 1616)], order=2)                                  # the order it has
    assert ok["status"] == cp.NOT_MINIMUM_PHASE or ok["status"] == 0      # (poles on the unit circle: either side)
    assert abs(ok["coefs"][1] + 2 * math.cos(2 * math.pi / 8)) < 1e-3 and abs(ok["coefs"][2] - 1.0) < 1e-3


def test_a_growing_response_is_not_minimum_phase_and_keeps_its_taps():
    """x[n] = round(1.02^n * cos): the free response of a filter with poles at radius 1.02"""
    n = np.arange(300)
    x = np.round(40.0 * 1.02 ** n * np.cos(0.7 * n)).astype(np.int16)
    assert np.abs(x).max() < 32767
    r = one(x, [(20, 300)], order=2)
    want = [1.0, -2 * 1.02 * math.cos(0.7), 1.02 ** 2]
    assert r["status"] == cp.NOT_MINIMUM_PHASE
    assert np.abs(r["coefs"] - want).max() < 1e-3 and np.isfinite(r["err"]) and r["err"] / r["r0"] < 1e-5
    assert not tr.reflection(r["coefs"])[1]


def test_garbage_records_read_nothing_out_of_range():
    """negative, huge, period 0, status != 0, C > cycles_pitch: the row is a slice of a poisoned buffer, and the
    restatement hands that slice alone to the steps that read samples -- an index outside it would raise or, negative,
    read the slice's own end, which the poisoned copy below would show"""
    rng = np.random.default_rng(9)
    n, p = 700, 8
    body = rng.integers(-2000, 2000, n).astype(np.int16)
    big = 2 ** 31 - 1
    Cy = np.zeros((1, 12), dtype=gl.CYCLE_DTYPE)
    Cy["close"][0] = [-big - 1, -5, big, n - 3, 100, 200, 300, 400, 500, -4, n - 50, 50]
    Cy["period"][0] = [big, 600, big, 40, 0, -7, 60, 60, big, 30, 60, 90]
    Cy["status"][0] = [0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0]
    for f in ("gci", "peak"):
        Cy[f][0] = Cy["close"][0]
    R = np.zeros(1, dtype=gl.REC_DTYPE)
    results = []
    for poison in (32767, -12345):
        buf = np.full(n + 2000, poison, dtype=np.int16)
        buf[1000:1000 + n] = body
        row = buf[1000:1000 + n]
        for count, rejected in ((12, 0), (7, 90), (big, big)):
            R["n_cycles"], R["n_rejected"] = count, rejected
            res = cp.analyse(row[None, :], 16000, R, Cy, order=p, delay=4, span_q=256)
            results.append((res["spans"][0][0], res["coefs"].tobytes(), res["counts"].tobytes()))
    half = len(results) // 2
    assert results[:half] == results[half:]                                # the poison was never read
    assert results[0][0] == [(404, 464), (0, 30), (54, 144)]
    for status in (gl.GL_NO_CYCLES, gl.GL_BAD_MARKS, gl.GL_BAD_MARKS | gl.GL_REJECTED):
        R["status"] = status
        assert cp.analyse(body[None, :], 16000, R, Cy, order=p, delay=4, span_q=256)["counts"][0, 0, 0] == 0
    R["status"] = 0
    R["n_cycles"], R["n_rejected"] = -20, 5
    assert cp.analyse(body[None, :], 16000, R, Cy, order=p, delay=4, span_q=256)["counts"][0, 0, 0] == 0


# 4 ---- the acceptance rule

def test_acceptance_at_its_edges():
    rng = np.random.default_rng(4)
    n, p = 600, 10
    x = rng.integers(-2000, 2000, n).astype(np.int16)
    b, e = 100, 180

    def pooled(xx, span, **kw):
        return one(xx, [span], order=p, **kw)["counts"][0]

    assert pooled(x, (b, e)) == 1
    for at, value, keeps in ((b, 32767, 0), (e - 1, -32767, 0), (b - 1, 32767, 1), (e, -32767, 1), (b + 5, -32768, 0),
                             (b + 5, 32766, 1), (b + 5, -32766, 1)):
        y = x.copy()
        y[at] = value
        assert pooled(y, (b, e)) == keeps, (at, value)
    assert pooled(x, (n - 50, n)) == 1 and pooled(x, (n - 49, n + 1)) == 0          # e == len, e == len + 1
    assert pooled(x, (0, 40)) == 1 and pooled(x, (-1, 40)) == 0                    # b == 0, b == -1
    assert pooled(x, (50, 50 + p + 1), min_equations=p) == 1                       # e - b == p + 1: one equation pooled
    assert one(x, [(50, 50 + p + 1)], order=p)["counts"][1] == 1
    assert pooled(x, (50, 50 + p)) == 0
    # the span in 64-bit integers, anchor by anchor; span_q in 256ths, rounded down
    R, Cy = records([(0, 0)])
    Cy["close"], Cy["gci"], Cy["peak"], Cy["period"] = 200, 300, 400, 101
    for anchor, at in (("close", 200), ("gci", 300), ("peak", 400)):
        res = cp.analyse(x[None, :], 16000, R, Cy, order=p, anchor=anchor, delay=-7, span_q=77)
        assert res["spans"][0][0] == [(at - 7, at - 7 + (77 * 101) // 256)]


# 5 ---- frames

def test_framed_mode_pools_the_spans_inside_each_frame():
    rng = np.random.default_rng(5)
    fs, n, p = 16000, 4000, 4
    x = rng.integers(-2000, 2000, n).astype(np.int16)
    kw = dict(order=p, window_s=0.05, hop_s=0.025, delay=4, span_q=256)      # L 800, H 400: starts 0, 400, ..., 3200
    spans = [(0, 60), (400, 460), (1140, 1200), (1141, 1201), (1199, 1260), (2000, 2100), (3940, 4000)]
    R, Cy = records(spans)
    res = cp.analyse(x[None, :], fs, R, Cy, **kw)
    L, H, starts = lr.frame_plan(fs, n, lr.opts(order=p, window=lr.RECTANGULAR, window_s=0.05, hop_s=0.025))
    assert (L, H) == (800, 400) and res["n_frames"][0] == len(starts) == 9 and list(res["start"][0]) == starts
    want = {0: [(0, 60), (400, 460)], 1: [(400, 460), (1140, 1200)], 2: [(1140, 1200), (1141, 1201), (1199, 1260)],
            3: [], 4: [(2000, 2100)], 5: [(2000, 2100)], 6: [], 7: [], 8: [(3940, 4000)]}
    for j in range(9):
        assert res["spans"][0][j] == want[j], j                            # b == s_j and e == s_j + L are inside
        assert res["counts"][0, j, 0] == len(want[j])
        alone = one(x, want[j], order=p)
        assert res["coefs"][0, j].tobytes() == alone["coefs"].tobytes() and res["status"][0, j] == alone["status"]
    # the frame plan the C helper gives is lpc_ref's
    lo = vs.cplpc_lpc_opts(**{k: v for k, v in kw.items() if k in ("order", "window_s", "hop_s")})
    assert (lo["window_s"], lo["hop_s"], lo["pre_emphasis"], lo["order"]) == (0.05, 0.025, 0, p)
    for length in (0, 799, 800, 1199, 1200, 4000, 4399):
        plan = lr.frame_plan(fs, length, lr.opts(**lo))
        assert vs.lpc_frames(fs, length, **lo) == len(plan[2]) == vs.cplpc_frames(fs, length, order=p, window_s=0.05,
                                                                                  hop_s=0.025)
    assert vs.cplpc_frames(fs, 0) == 1 and vs.cplpc_frames(fs, 123456) == 1
    assert tuple(vs.inverse_from_lpc(fs, n, "hold", **lo))[:4] == (9, 400, 200, n)


def test_the_equation_count_stops_short_of_two_to_the_31():
    spans = [(0, 2 ** 30 + 5)] * 3
    got, n_eq = cp.pooled(spans, 0, 2 ** 31 - 1, 5)
    assert len(got) == 1 and n_eq == 2 ** 30


# 6 ---- what it is for

# |closed-phase - flow| per quantity, the largest over the three rows, as test_closed_phase_sets_reach_the_flow printed it
PRINTED_GAPS = {"shimmer": 7.09e-05, "oq": 2.97e-06, "qoq": 2.04e-04, "naq": 6.00e-05}


@pytest.mark.parametrize("args,f0_min", [(("-s", "2"), 50.0), (("-s", "5", "-j", "2"), 50.0), (("-s", "10"), 70.0)])
def test_closed_phase_sets_reach_the_flow(args, f0_min):
    """tools/cplpc_table.py's set-up: 16 oracle vowels -v a, F0 100, 22050 Hz, 1 s, seeds 300..315, order 22; first pass
    IAIF -> inverse (hold, 0.99, 1/10) -> measure -> glottal 26 / 128; second pass at de-emphasis 1.  Printed by this
    test (mean over the 16 rows; the yardstick is the oracle's flow):

        flowgen args          signal                      shimmer  OQ      QOQ     NAQ      |closed-phase - flow|
        -s 2                  flow                        0.0203   0.3955  0.2545  0.1358
                              IAIF sets (de-emphasis 1)   0.0290   0.4163  0.2637  0.1434
                              closed-phase sets           0.0203   0.3955  0.2545  0.1357   7.39e-07 0 0 5.48e-05
        -s 5 -j 2             flow                        0.0505   0.4091  0.2633  0.1404
                              IAIF sets (de-emphasis 1)   0.0834   0.4275  0.2734  0.1412
                              closed-phase sets           0.0505   0.4091  0.2635  0.1404   4.86e-06 2.97e-06 2.04e-04 4.63e-05
        -s 10, f0_min 70      flow                        0.1017   0.3831  0.2466  0.1315
                              IAIF sets (de-emphasis 1)   0.1187   0.4076  0.2570  0.1378
                              closed-phase sets           0.1016   0.3831  0.2467  0.1314   7.09e-05 0 1.49e-04 6.00e-05

    err / r0 of the 48 sets: 7.2e-09 .. 7.3e-08; max |a_j - table| 0.009 .. 0.065.  Printed only (tools/cplpc_table.py):
    -s 10 with the default f0_min 50, where one row of 16 is marked at every other cycle (period 440), its set is off by
    3.7 and its err / r0 is 8.5e-06; and flowgen -n 20, where the closed phase carries noise and the method fails (err /
    r0 0.3, shimmer 0.07 for 0.018 on the flow).

    Asserted for each row: every set at status 0; |closed-phase - flow| < |IAIF - flow| for shimmer, OQ, QOQ and NAQ;
    each closed-phase gap within twice the largest printed one (PRINTED_GAPS)."""
    import cplpc_table
    t = cplpc_table.table(tuple(args), f0_min)
    cplpc_table.show(" ".join(args), t)
    assert (t["status"] == 0).all()
    for q in cplpc_table.QUANTITIES:
        gap, other = abs(t["closed"][q] - t["flow"][q]), abs(t["iaif"][q] - t["flow"][q])
        print("%-8s gap closed-phase %.2e, IAIF %.2e" % (q, gap, other))
        assert gap < other, q
        assert gap <= 2 * PRINTED_GAPS[q], q


# 7 ---- the host helpers of the C ABI (no device)

def test_defaults_and_refusals():
    lib = vs.load()
    o = _ffi.CplpcOpts()
    assert C.sizeof(_ffi.CplpcOpts) == 56 == cp.OPTS_DTYPE.itemsize
    assert lib.vs_cplpc_defaults(None) == _ffi.VS_ERR_ARG and lib.vs_cplpc_defaults(C.byref(o)) == 0
    assert (o.order, o.anchor, o.delay, o.span_q, o.min_equations, o.n_formants, o.reserved_) == (22, 0, 4, 77, 0, 5, 0)
    assert (o.window_s, o.hop_s, o.f_lo) == (0.0, 0.010, 50.0)
    assert {vs.VS_CP_FEW_EQUATIONS, vs.VS_CP_SINGULAR, vs.VS_CP_NOT_MINIMUM_PHASE} == {0x10, 0x20, 0x40}
    lo = _ffi.LpcOpts()
    n = C.c_int32()

    def rc(**kw):
        reserved = kw.pop("reserved_", 0)
        oo = vs.cplpc_opts(**kw)
        oo.reserved_ = reserved
        a = lib.vs_cplpc_lpc_opts(C.byref(oo), C.byref(lo))
        assert lib.vs_cplpc_frames(C.byref(oo), 16000, 16000, C.byref(n)) in (a, _ffi.VS_ERR_RANGE)
        return a

    assert lib.vs_cplpc_lpc_opts(None, None) == _ffi.VS_ERR_ARG and lib.vs_cplpc_frames(None, 16000, 100, None) == _ffi.VS_ERR_ARG
    assert lib.vs_cplpc_lpc_opts(None, C.byref(lo)) == 0 and lib.vs_cplpc_frames(None, 16000, 100, C.byref(n)) == 0 and n.value == 1
    for kw in (dict(), dict(order=1), dict(order=40), dict(anchor="gci"), dict(anchor="peak"), dict(delay=-32768),
               dict(delay=32767), dict(span_q=1), dict(span_q=256), dict(min_equations=22), dict(n_formants=0),
               dict(window_s=0.025)):
        assert rc(**kw) == 0, kw
    for kw in (dict(order=0), dict(order=41), dict(anchor=3), dict(anchor=-1), dict(delay=-32769), dict(delay=32768),
               dict(span_q=0), dict(span_q=257), dict(min_equations=21), dict(min_equations=-1), dict(window_s=-0.01)):
        assert rc(**kw) == _ffi.VS_ERR_RANGE, kw
    for kw in (dict(reserved_=1), dict(n_formants=21), dict(n_formants=-1), dict(f_lo=-1.0), dict(hop_s=-0.01),
               dict(window_s=math.nan), dict(hop_s=math.inf)):
        assert rc(**kw) == _ffi.VS_ERR_ARG, kw
    # a window no frame fits is the row's refusal, as for vs_lpc_frames
    oo = vs.cplpc_opts(window_s=0.0001)
    assert lib.vs_cplpc_frames(C.byref(oo), 16000, 16000, C.byref(n)) == _ffi.VS_ERR_RANGE
    assert lib.vs_cplpc_frames(C.byref(vs.cplpc_opts()), 0, 100, C.byref(n)) == _ffi.VS_ERR_RANGE
    # the launch refuses the same before it touches a device: no context, no buffers
    assert lib.vs_cplpc_launch(None, None, None, 0, 0, 0, None, None, None, None, 0, 0, None, None, None, None) == _ffi.VS_ERR_ARG
    assert lib.vs_cplpc(None, None, None, 0, 0, 0, None, None, None, None, 0, 0, None, None, None, None) == _ffi.VS_ERR_ARG


def test_the_printed_line():
    stat = np.zeros(1, dtype=[("n_unusable", "<i4"), ("n_clipped", "<i4")])[0]
    assert cp.format_line("f.wav", stat, [[3, 90]], [4.0], [1e-7], [0]) == "f.wav 1 0 0 3 90 2.500e-08 0"
    assert cp.format_line("f.wav", stat, [[3, 90], [0, 0]], [4.0, 0.0], [1e-7, math.nan], [0, 16]) == "f.wav 2 0 0 3 90 2.500e-08 16"
    assert cp.format_line("f.wav", stat, [[0, 0]], [0.0], [math.nan], [16]) == "f.wav 1 0 0 0 0 nan 16"
    assert cp.format_set([1.0, -0.5, math.nan]) == "# set 1 -0.5 nan"
