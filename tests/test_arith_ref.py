"""The numpy restatements of the two opt-in arithmetics of the synthesis filter (tests/arith_ref.py) on the CPU: the
float32 fma they are built on against exact rational arithmetic; the FMA form equal to the track restatement's (hold,
one set); the single-precision form reproducing, figure for figure, what tests/golden/f32_bounds.json recorded of the
device -- so the order written down in include/voice_synth.h is the order the MI355X ran when the fixture was measured.

The second half builds the cases of tests/test_gpu_arith.py -- table lanes, clustered custom sets, lanes whose every odd
flow sample is a rounding tie, such lanes with taps that tell the FMA form from the exact one, lanes that saturate --
with the conditions under which those comparisons mean something, asserted from the restatements alone.  The GPU tests
take the cases and the expected bytes from here."""
import ctypes as C
import fractions
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import arith_ref as ar  # noqa: E402
import track_ref as tr  # noqa: E402

TABLES = "aiu1234567"
F = fractions.Fraction


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _round_to_float32(q):
    """the float32 nearest the Fraction q, ties to even (float() of a Fraction rounds once, to double: one of that
    double's float32 neighbours is the answer)"""
    d = np.float32(float(q))
    cands = (np.nextafter(d, np.float32(-np.inf)), d, np.nextafter(d, np.float32(np.inf)))
    return float(min(cands, key=lambda v: (abs(F(float(v)) - q), int(np.float32(v).view(np.uint32)) & 1)))


# ---- what the restatements are built on ------------------------------------------------------------------------------

def test_float32_fma_is_the_exactly_rounded_one():
    """three families of 6000 triples against fractions.Fraction: drawn operands; c within a few float32 ulps of -a*b
    (heavy cancellation); and a*b a float32 rounding midpoint (3 times an odd 24-bit integer that stays under 2^25)
    with c zero or far below the last bit of a double sum -- where the sum rounded to double first and to float32 second
    goes to the even neighbour whatever the sign of c"""
    rng = np.random.default_rng(71)
    n = 6000
    scale = lambda lo, hi, m: 2.0 ** rng.integers(lo, hi, m)          # noqa: E731
    a = _f32(rng.uniform(-2, 2, 3 * n) * scale(-20, 20, 3 * n))
    b = _f32(rng.uniform(-2, 2, 3 * n) * scale(-20, 20, 3 * n))
    c = _f32(rng.uniform(-2, 2, 3 * n) * scale(-40, 40, 3 * n))
    near = _f32(-(a[n:2 * n] * b[n:2 * n])).astype(np.float32)
    for _ in range(3):                                                # 0..3 ulps away, either side
        side = rng.choice([-np.inf, np.inf], n).astype(np.float32)
        near = np.where(rng.integers(0, 2, n) == 1, np.nextafter(near, side), near)
    c[n:2 * n] = near
    odd = (rng.integers(2 ** 22, 11184810 // 2, n) * 2 + 1).astype(np.float64)     # 2^23 < odd, 3 * odd < 2^25
    s = scale(-30, 30, n)
    a[2 * n:], b[2 * n:] = 3.0 * rng.choice([-1.0, 1.0], n), odd * s
    c[2 * n:] = rng.choice([-1.0, 0.0, 1.0], n) * s * scale(-80, -30, n)
    assert np.array_equal(_f32(a), a) and np.array_equal(_f32(b), b) and np.array_equal(_f32(c), c)
    got = ar.fmaf(a, b, c)
    want = np.array([_round_to_float32(F(float(x)) * F(float(y)) + F(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    twice = _f32(a * b + c)                       # ... and rounding twice is another function on the last two families
    print("float32 fma: %d triples exact; rounding the double sum differs on %d cancelling and %d midpoint triples" % (
        3 * n, (twice[n:2 * n] != want[n:2 * n]).sum(), (twice[2 * n:] != want[2 * n:]).sum()))
    assert (twice[2 * n:] != want[2 * n:]).sum() > n // 8


def test_the_three_roundings():
    """on halves, their neighbours and the clamp, against integer arithmetic on Fractions; round2int is held to the
    oracle's by tests/test_track_ref.py"""
    halves = np.arange(-70, 70) / 2.0
    x = np.concatenate([halves, np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf),
                        [32766.5, 32767.5, -32767.5, -32768.5, 1e9, -1e9, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31 - 1, -0.0],
                        np.random.default_rng(72).uniform(-40000, 40000, 2000)])
    clamp = lambda v: max(-32767, min(32767, v))                      # noqa: E731
    up = [clamp(math.floor(F(float(v)) + F(1, 2))) for v in x]
    even = [clamp(round(F(float(v)))) for v in x]                     # Python rounds a Fraction's ties to even
    assert ar.half_up(x).tolist() == up and ar.nearest_even(x).tolist() == even
    assert ar.half_up([np.nan])[0] == 0 and ar.nearest_even([np.nan])[0] == 0
    ties = halves[1::2]
    assert (ar.half_up(ties) - tr.round2int(ties) == 1).all()         # round2int takes a half downwards
    assert np.array_equal(ar.rounded(x, "round2int"), tr.round2int(x))


def _rows(n, length, gain, pre):
    rows = np.zeros(n, dtype=tr.ROW_DTYPE)
    rows["n_sets"], rows["hop"], rows["length"], rows["gain"], rows["pre_emphasis"] = 1, 1, length, gain, pre
    return rows


def test_filter_fma_is_the_track_restatement_with_one_set():
    n = 600
    lanes = [vs.lane_from_cli(FLOWGEN3, ["-v", v, "-g", "%g" % (1 + 0.7 * k), "-p", ["1", "0", "0.37"][k % 3]], 7 + k)[0]
             for k, v in enumerate(TABLES)]
    flow = pyoracle.source(lanes, n)
    A, gain, pre = lane_sets(lanes)
    want, _ = tr.filter_track(flow, A[:, None, :], _rows(10, n, gain, pre), tr.HOLD, arith="fma")
    got = ar.filter_fma(flow, A, gain, pre, "round2int")
    assert np.array_equal(got, want) and np.abs(want.astype(np.int32)).max() > 1000


def test_filter_f32_reproduces_the_device_measurements():
    """the lanes of tools/f32_survey.py, 64 x 16000 per case, against the exact oracle: the ten tables at the
    reference's defaults and all four settings of table '5' give the figures the fixture recorded on the device"""
    import f32_survey
    bounds = json.load(open(os.path.join(ROOT, "tests", "golden", "f32_bounds.json")))["cases"]
    keys = ["%s/10/1" % v for v in TABLES] + ["5/%s/%s" % s for s in f32_survey.SETTINGS if s != ("10", "1")]
    assert len(keys) == 13 and len(set(keys)) == 13
    lanes = [lane for key in keys for lane in f32_survey.case_lanes(*key.split("/"))]
    flow = pyoracle.source(lanes, 16000)
    want = pyoracle.synth(lanes, 16000)
    assert np.array_equal(want, pyoracle.filter(lanes, flow))
    A, gain, pre = lane_sets(lanes)
    got, smallest = ar.filter_f32(flow, A, gain, pre)
    assert smallest > ar.F32_MIN_NORMAL
    for i, key in enumerate(keys):
        pc, mx, rms = f32_survey.stats(got[64 * i:64 * i + 64], want[64 * i:64 * i + 64])
        mine = {"pct": round(pc, 2), "max": mx, "rms": float("%.3e" % rms)}
        print("%-8s restated %s  recorded %s" % (key, mine, bounds[key]))
        assert mine == {k: bounds[key][k] for k in ("pct", "max", "rms")}, (key, mine, bounds[key])


# ---- the cases of tests/test_gpu_arith.py ----------------------------------------------------------------------------

NS = 1000                    # 41 whole super-steps of 24 and a tail of 16
SAMPLE_COUNTS = (1, 23, 24, 25, 47, 48, 49, 999, 1000)
BATCH = 130                  # two whole groups of 64 utterances and a ragged one
PREFIXES = (1, 63, 65, BATCH)
FLOWGEN3 = ["-r", "16000", "-d", "1", "-j", "1", "-s", "5.76", "-n", "20"]           # config 3's source options
TABLE_GAINS = ("1", "10", "20")
TABLE_PRES = ("1", "0", "0.5", "0.37")
# pole pairs of radius r at angles within +-spread of one another (tests/test_gpu_track_hostile.py, _clustered_set).  A
# lane's gain must be at least 1 (vs_lane_validate, as vowel_new.c:132), where a track row's may be 1e-7: the radius
# comes down from r in steps of 0.02 until the set's peak at gain 1 is under CLUSTER_PEAK, and the gain takes it there
CLUSTERS = {12: (0.99, 0.005), 22: (0.9, 0.1)}
CLUSTER_PEAK = 20000.0
# all taps zero and this gain: every odd flow sample lands on k + 0.5 (0.5 itself is no lane's gain, see above)
TIE_GAIN = 1.5
# the tie lanes with two or three EVEN taps of this size on top.  Each product is 0.2 to 0.4 of the last bit of x*gain:
# the exact form subtracts them from x*gain one by one and every difference rounds back to the tie, which round2int
# takes downwards; the FMA form collects the even taps in a partial sum of their own, which moves x*gain by a whole
# last bit once it passes half of one -- off the tie, upwards in every rounding
SPLIT_TAP = -0.2 * 2.0 ** -52
SPLIT_TAPS = ((2, 4), (2, 6), (4, 8), (2, 4, 6))
N_TABLE, N_LONG, N_CLUSTER, N_SPLIT, N_TIE, N_SAT = 72, 6, 8, 8, 24, 12
assert N_TABLE + N_LONG + N_CLUSTER + N_SPLIT + N_TIE + N_SAT == BATCH


def long_period_flowgen(k):
    """config 5's source options near the low end of its F0 sweep: periods of 186 and 173 samples (two of them, so
    that a group's cosine rows stay few and four rings still share a workgroup's LDS)"""
    f0 = (86.0, 92.0)[k % 2]
    return ["-r", "16000", "-d", "1", "-f", "%.2f" % f0, "-g", "%.2f" % round(f0 * 125.0 / 120.0 + 1.0, 2), "-j", "1",
            "-s", "5.76", "-n", "20"]


def _plain_peaks(sets, x, pre):
    """largest |y[n] - pre*y[n-1]| of 1/A(z) on x at gain 1 for each of sets [K][order+1], in plain double arithmetic"""
    K, N, p = len(sets), len(x), sets.shape[1] - 1
    Y = np.zeros((K, N + p))
    for n in range(N):
        Y[:, n + p] = x[n] - (sets[:, 1:] * Y[:, n:n + p][:, ::-1]).sum(axis=1)
    return np.abs(Y[:, p:] - pre * Y[:, p - 1:-1]).max(axis=1)


def clustered_set(order, rng, x, pre):
    """order // 2 pole pairs at angles within +-spread of one another, at the largest radius r, r - 0.02, .. whose
    filter keeps the flow x under CLUSTER_PEAK at gain 1"""
    r, spread = CLUSTERS[order]
    centre = rng.uniform(1.0, 2.1)
    angles = centre + rng.uniform(-spread, spread, order // 2)
    sets = []
    for k in range(40):
        z = (r - 0.02 * k) * np.exp(1j * angles)
        A = np.real(np.poly(np.concatenate([z, np.conj(z)])))
        A[0] = 1.0
        sets.append(A)
    sets = np.array(sets)
    x = x.astype(np.float64)               # (at the lane's own pre-emphasis and at 1, which batch(True) gives it)
    ok = np.flatnonzero(np.maximum(_plain_peaks(sets, x, pre), _plain_peaks(sets, x, 1.0)) * 1.01 < CLUSTER_PEAK)
    return sets[ok[0]]


def lane_sets(lanes):
    """(A [lanes][23], gain, pre) of table and custom lanes of at most 22 taps: zeros in the missing taps"""
    A = np.zeros((len(lanes), ar.ORDER + 1))
    for i, l in enumerate(lanes):
        if l.vowel == 0:
            assert l.order <= ar.ORDER
            A[i, :l.order + 1] = l.A[:l.order + 1]
        else:
            A[i] = vs.vowel_coefficients(chr(l.vowel))
    A[:, 0] = 1.0
    return A, np.array([l.gain for l in lanes], dtype=np.float32), np.array([l.pre_emphasis for l in lanes], dtype=np.float32)


class Case(dict):
    """one batch and what the restatements make of it: lanes (a vs.Lane array), kinds (a name per lane), flow (the
    oracle's, read-only), A / gain / pre, o_fma (the FMA form before its rounding), f32 (the single-precision PCM),
    f32_smallest"""
    __getattr__ = dict.__getitem__

    def rows(self, kind):
        return np.flatnonzero(self.kinds == kind)

    def fma(self, rounding, lanes=BATCH, ns=NS):
        return ar.rounded(self.o_fma[:lanes, :ns], rounding)


@functools.lru_cache(maxsize=None)
def _proto_lanes():
    """(kind, lane) for the 130 lanes, kind by kind"""
    out = []
    for i in range(N_TABLE):
        va = ["-v", TABLES[i % 10], "-g", TABLE_GAINS[i % 3], "-p", TABLE_PRES[(i + i // 20) % 4]]
        out.append(("table", vs.lane_from_cli(FLOWGEN3, va, 300 + i)[0]))
    for i in range(N_LONG):
        va = ["-v", TABLES[(3 * i + 1) % 10], "-g", TABLE_GAINS[i % 3], "-p", TABLE_PRES[i % 4]]
        out.append(("long", vs.lane_from_cli(long_period_flowgen(i), va, 400 + i)[0]))
    rng = np.random.default_rng(622)
    for i in range(N_CLUSTER):
        lane = vs.lane_from_cli(FLOWGEN3, ["-v", "a", "-g", "1", "-p", TABLE_PRES[i % 4]], 500 + i)[0]
        A = clustered_set(22 if i % 2 == 0 else 12, rng, pyoracle.source([lane], NS)[0], lane.pre_emphasis)
        out.append(("cluster", vs.set_coefficients(lane, A)))
    for i in range(N_SPLIT):
        lane = vs.lane_from_cli(FLOWGEN3, ["-v", "a", "-g", "%g" % TIE_GAIN, "-p", "0"], 550 + i)[0]
        A = np.concatenate([[1.0], np.zeros(22)])
        A[list(SPLIT_TAPS[i % len(SPLIT_TAPS)])] = SPLIT_TAP
        out.append(("split", vs.set_coefficients(lane, A)))
    for i in range(N_TIE):
        lane = vs.lane_from_cli(FLOWGEN3 if i % 4 else long_period_flowgen(i // 4), ["-v", "a", "-g", "%g" % TIE_GAIN, "-p", "0"], 600 + i)[0]
        out.append(("tie", vs.set_coefficients(lane, np.concatenate([[1.0], np.zeros(22)]))))
    for i in range(N_SAT):
        va = ["-v", TABLES[(7 * i) % 10], "-g", "30" if i % 3 == 2 else "1000", "-p", TABLE_PRES[i % 4]]
        out.append(("sat", vs.lane_from_cli(FLOWGEN3, va, 700 + i)[0]))
    return out


@functools.lru_cache(maxsize=None)
def batch(pre1):
    """the 130 lanes, the kinds dealt through the batch so that every prefix holds several of them.  pre1: every lane
    at pre-emphasis 1, which selects the kernels' instantiation for that case"""
    proto = _proto_lanes()
    order = [(37 * i) % BATCH for i in range(BATCH)]
    assert sorted(order) == list(range(BATCH))
    kinds = np.array([proto[j][0] for j in order])
    lanes = (vs.Lane * BATCH)()
    for i, j in enumerate(order):
        C.memmove(C.byref(lanes[i]), C.byref(proto[j][1]), C.sizeof(vs.Lane))
        if pre1:
            lanes[i].pre_emphasis = 1.0
    flow = pyoracle.source(lanes, NS)
    flow.setflags(write=False)
    # the clustered sets: the gain that takes the filter's peak to CLUSTER_PEAK (their lanes were made with -g 1)
    A, gain, pre = lane_sets(lanes)
    cl = np.flatnonzero(kinds == "cluster")
    peak = np.abs(ar.fma_unrounded(flow[cl], A[cl], gain[cl], pre[cl])).max(axis=1)
    for r, pk in zip(cl, peak):
        lanes[r].gain = float(np.float32(CLUSTER_PEAK / pk))
    A, gain, pre = lane_sets(lanes)
    o = ar.fma_unrounded(flow, A, gain, pre)
    f32, smallest = ar.filter_f32(flow, A, gain, pre)
    for a in (o, f32, kinds):
        a.setflags(write=False)
    return Case(lanes=lanes, kinds=kinds, flow=flow, A=A, gain=gain, pre=pre, o_fma=o, f32=f32, f32_smallest=smallest)


def saturated(pcm):
    return np.abs(pcm.astype(np.int32)) == 32767


def check_batch_conditions(c, pre1):
    """the conditions under which a byte-for-byte comparison on this batch tells a right kernel from a wrong one;
    returns the lines for the profile"""
    lines = []
    lib = vs.load()
    assert len(c.lanes) == BATCH and all(l.out_snr == 0.0 for l in c.lanes)
    assert all(lib.vs_lane_validate(C.byref(l)) == 0 for l in c.lanes)       # lanes a plan accepts
    assert all((l.pre_emphasis == 1.0) for l in c.lanes) == pre1
    assert np.isfinite(c.o_fma).all() and c.f32_smallest > ar.F32_MIN_NORMAL, c.f32_smallest   # (0: not finite)
    for k in PREFIXES[:-1]:                      # every prefix but the first holds at least four kinds of lanes
        assert len(set(c.kinds[:k])) >= min(k, 4), (k, c.kinds[:k])
    exact = pyoracle.filter(c.lanes, c.flow)
    r2i, even, up = (c.fma(r) for r in ar.ROUNDINGS)
    # the clustered sets: as ill-conditioned as a lane's gain allows, loud, not saturated
    cl = c.rows("cluster")
    peak = np.abs(exact[cl].astype(np.int32)).max(axis=1)
    assert not saturated(exact[cl]).any() and peak.min() > CLUSTER_PEAK / 2 and (c.gain[cl] >= 1.0).all(), (peak, c.gain[cl])
    lines.append("clustered sets: radii %s, largest tap %.0f, gains %.2f..%.2f, peaks %d..%d; FMA form differs from the exact "
                 "oracle in %d of %d samples" % (
                     " ".join("%.2f" % np.abs(np.roots(c.A[r, :c.lanes[r].order + 1])).max() for r in cl), np.abs(c.A[cl]).max(),
                     c.gain[cl].min(), c.gain[cl].max(), peak.min(), peak.max(), (r2i[cl] != exact[cl]).sum(), exact[cl].size))
    # the split-sum lanes tell the FMA form from the exact one
    sp = c.rows("split")
    differs = r2i[sp] != exact[sp]
    assert differs.sum() >= 10 and differs.any(axis=1).sum() >= 3, (differs.sum(), differs.any(axis=1).sum())
    assert np.abs(r2i[sp].astype(np.int32) - exact[sp]).max() == 1 and not saturated(exact[sp]).any()
    lines.append("split-sum lanes: FMA form differs from the exact oracle in %d of %d samples on %d of %d rows (by 1 LSB)" % (
        differs.sum(), differs.size, differs.any(axis=1).sum(), len(sp)))
    others = np.flatnonzero((c.kinds != "cluster") & (c.kinds != "split"))
    lines.append("every other lane: FMA form differs from the exact oracle in %d of %d samples" % (
        (r2i[others] != exact[others]).sum(), r2i[others].size))
    # saturating lanes: some samples clamp and some do not, in both arithmetics
    for name, pcm in (("fma", r2i), ("f32", c.f32)):
        sat = saturated(pcm[c.rows("sat")])
        assert sat.any(axis=1).all() and not sat.all(axis=1).any(), (name, sat.mean(axis=1))
        lines.append("saturating lanes, %s: %.1f %% of the samples at the clamp (per lane %.1f .. %.1f %%)" % (
            name, 100 * sat.mean(), 100 * sat.mean(axis=1).min(), 100 * sat.mean(axis=1).max()))
    # the tie lanes tell the three roundings apart
    if not pre1:
        t = c.rows("tie")
        assert not c.A[t, 1:].any() and (c.gain[t] == TIE_GAIN).all() and (c.pre[t] == 0.0).all()
        oddx = (c.flow[t] & 1) == 1
        assert np.array_equal(c.o_fma[t], c.flow[t] * TIE_GAIN)
        pairs = {"round2int / nearest even": r2i[t] != even[t], "round2int / half up": r2i[t] != up[t],
                 "nearest even / half up": even[t] != up[t]}
        for name, d in pairs.items():
            assert d.mean() >= 0.10 and (d.mean(axis=1) >= 0.10).all(), (name, d.mean(axis=1))
            assert not (d & ~oddx).any()
        assert np.array_equal(c.f32[t], up[t])   # an exact product and sums with zero: nothing rounds before the tie
        lines.append("tie lanes: %.1f %% of the flow samples odd; the roundings differ in %s of the samples" % (
            100 * oddx.mean(), ", ".join("%.1f %% (%s)" % (100 * d.mean(), n) for n, d in pairs.items())))
    # the two FMA families differ beyond the tie lanes too; single precision is another function altogether
    lines.append("whole batch: round2int / nearest even differ in %d samples, FMA nearest even / single precision in %d of %d; "
                 "smallest non-zero single-precision intermediate %.3e" % (
                     (r2i != even).sum(), (even != c.f32).sum(), even.size, c.f32_smallest))
    assert (even != c.f32).mean() > 0.01
    return lines


@pytest.mark.parametrize("pre1", [False, True])
def test_batch_conditions(pre1):
    for line in check_batch_conditions(batch(pre1), pre1):
        print("%s: %s" % ("pre-emphasis 1" if pre1 else "mixed         ", line))


def test_the_oracle_flow_of_a_shorter_call_is_a_prefix():
    """the expected bytes of every sample count are prefixes of the 1000-sample restatement: the flow must be one"""
    c = batch(False)
    for ns in SAMPLE_COUNTS:
        assert np.array_equal(pyoracle.source(c.lanes, ns), c.flow[:, :ns]), ns
