"""The hostile batches of the synthesis filter kernels (tests/test_gpu_synth_hostile.py) and the conditions under which
a byte-for-byte comparison on them means something, built and asserted on the CPU from the restatements alone
(tests/arith_ref.py), in the style of tests/test_arith_ref.py.

Two batches of 130 lanes, every lane an explicit coefficient set on config 3's source options:
  H22 (orders 1, 2, 5, 12, 21, 22: the fused and the one-wave kernels; a mixed pre-emphasis variant and an all-1 one) and
  H40 (orders 1 .. 40, so the plan is wide and every lane runs the 40-tap form).
The kinds of lanes, dealt through the batch by a pattern of 13 so that every prefix holds several:
  loud        stable reflection-drawn sets (hostile_signals.reflection_sets) at three gains: the argument of the rounding
              passes int16, int32 and int64;
  tame        configs.random_pole_set at gains 1..10;
  neighbour   a tame set of order 5 right behind an unstable lane of order 1;
  tie, split  as in tests/test_arith_ref.py; in H40 the split taps sit above tap 22;
  unstable    a_1 = +-4 at order 1, and stable sets with every radius scaled past 1: the state leaves the doubles
              between NS/4 and 3 NS/4;
  unstable32  the same at a_1 = +-1.2 and smaller radii: the single-precision state leaves float32 in that window (in
              double these rows stay finite; the unstable ones leave float32 early).
What is promised of a lane ends at the first state that is not finite (include/voice_synth.h): f, per row and
arithmetic, is what the GPU tests compare up to.  profiles/synth_hostile_sets.txt keeps the lines printed here."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arith_ref as ar  # noqa: E402
import hostile_signals as hs  # noqa: E402
import test_arith_ref as cases  # noqa: E402
import track_ref as tr  # noqa: E402
from test_arith_ref import FLOWGEN3, SPLIT_TAP, TABLE_PRES, TIE_GAIN, long_period_flowgen  # noqa: E402

NS = 1000
BATCH = 130                  # two whole groups of 64 utterances and a ragged one
PREFIXES = (1, 63, 65, BATCH)
SAMPLE_COUNTS = {22: (1, 23, 24, 25, 47, 48, 49, 999, 1000),      # around the fused kernels' super-step of 24
                 40: (1, 47, 48, 49, 95, 96, 97, 999, 1000)}      # around the wide kernel's of 48
ORDERS = {22: (1, 2, 5, 12, 21, 22), 40: (1, 2, 5, 21, 22, 23, 24, 30, 31, 39, 40)}
CASES = ("h22", "h22p1", "h40")
PATTERN = ("loud", "tame", "unstable", "neighbour", "loud", "tie", "split", "loud", "unstable32", "loud", "tame",
           "unstable", "loud")
assert BATCH % len(PATTERN) == 0
# the gains of the loud lanes: the bands of LOUD_BANDS must hold for them (check_conditions).  On config 3's flows the
# reflection-drawn sets peak at 3e3..1e5 at gain 1 (noise and square waves take them to 6e4..4e7), so the three gains
# are 16, 1e7 and 1e17 where such flows would have 1, 1e6 and 1e15
LOUD_GAINS = (16.0, 1e7, 1e17)
LOUD_BANDS = ((2.0 ** 15, 2.0 ** 31), (2.0 ** 31, 2.0 ** 53), (2.0 ** 63, np.inf))      # max |o| of a row, per gain
# an unstable lane's largest root: 1e3 (a flow sample times a gain) * r^n reaches the largest double (1.8e308) or
# float32 (3.4e38) at n = NS/2 for r = 10^(305/500) = 4.07 and r = 10^(35.5/500) = 1.18
UNSTABLE_A1 = {"unstable": 4.0, "unstable32": 1.2}
UNSTABLE_RADIUS = {"unstable": 4.0, "unstable32": 1.2}
UNSTABLE_ORDERS = {22: (2, 22), 40: (2, 22, 40)}
WINDOW = (NS // 4, 3 * NS // 4)
SPLIT_TAPS = {22: cases.SPLIT_TAPS, 40: ((24, 26), (2, 40), (30, 38, 40), (24, 40))}


def lane_sets(lanes, P):
    """(A [lanes][P+1], gain, pre, order) of table and custom lanes of at most P taps: zeros in the missing taps
    (tests/test_arith_ref.lane_sets for any P)"""
    A = np.zeros((len(lanes), P + 1))
    order = np.zeros(len(lanes), dtype=np.int64)
    for i, l in enumerate(lanes):
        if l.vowel == 0:
            order[i] = l.order if l.order else ar.ORDER
            assert order[i] <= P
            A[i, :order[i] + 1] = l.A[:order[i] + 1]
        else:
            order[i] = ar.ORDER
            A[i, :ar.ORDER + 1] = vs.vowel_coefficients(chr(l.vowel))
    A[:, 0] = 1.0
    return (A, np.array([l.gain for l in lanes], dtype=np.float32), np.array([l.pre_emphasis for l in lanes], dtype=np.float32),
            order)


class Case(dict):
    """one batch and what the restatements make of it.  lanes, kinds, P, flow (the oracle's, read-only), A / gain / pre /
    order; per arithmetic ("exact", "fma", and "f32" where P = 22): o[name] the argument of the rounding, f[name] the
    first sample of each row whose state is not finite (NS: none); exact: the oracle's PCM; f32_smallest: per row"""
    __getattr__ = dict.__getitem__

    def rows(self, kind):
        return np.flatnonzero(self.kinds == kind)

    def want(self, family, lanes=BATCH, ns=NS):
        """(pcm, f) of the first lanes and samples; family: "exact", one of ar.ROUNDINGS (the FMA form) or "f32" """
        if family == "exact":
            return self.exact[:lanes, :ns], self.f["exact"][:lanes]
        if family == "f32":
            return ar.half_up(self.o["f32"][:lanes, :ns]), self.f["f32"][:lanes]
        return ar.rounded(self.o["fma"][:lanes, :ns], family), self.f["fma"][:lanes]


def _lane(i, gain, pre, seed):
    fg = long_period_flowgen(i // 20) if i % 20 == 7 else FLOWGEN3
    return vs.lane_from_cli(fg, ["-v", "a", "-g", "%.2f" % gain, "-p", pre], seed)[0]


@functools.lru_cache(maxsize=None)
def _lanes(P):
    """(kinds, lanes) of the mixed pre-emphasis variant"""
    rng = np.random.default_rng(2200 + P)
    orders = ORDERS[P]
    kinds = np.array([PATTERN[i % len(PATTERN)] for i in range(BATCH)])
    lanes = (vs.Lane * BATCH)()
    count = {k: 0 for k in set(PATTERN)}
    for i, kind in enumerate(kinds):
        k = count[kind]
        count[kind] += 1
        pre = TABLE_PRES[i % 4]
        gain = 1.0
        order = orders[(i + i // len(orders) - 1) % len(orders)]     # (lane 0 has the most taps: every prefix of H40 is wide)
        if kind == "loud":
            A = hs.reflection_sets(rng, 1, 1, order)[0, 0]
        elif kind == "tame":
            A, gain = configs.random_pole_set(order, rng), rng.uniform(1, 10)
        elif kind == "neighbour":
            A, gain = configs.random_pole_set(5, rng), rng.uniform(1, 10)
        elif kind in ("tie", "split"):
            A, gain, pre = np.concatenate([[1.0], np.zeros(P)]), TIE_GAIN, "0"
            if kind == "split":
                A[list(SPLIT_TAPS[P][k % len(SPLIT_TAPS[P])])] = SPLIT_TAP
        else:                                    # every other unstable lane of order 1, a_1 of either sign
            if k % 2 == 0:
                A = np.array([1.0, UNSTABLE_A1[kind] * (1 if k % 4 == 0 else -1)])
            else:
                uo = UNSTABLE_ORDERS[P][(k // 2) % len(UNSTABLE_ORDERS[P])]
                stable = configs.random_pole_set(uo, rng)
                A = hs.scaled_radius(stable, UNSTABLE_RADIUS[kind] / np.abs(np.roots(stable)).max())
        lane = vs.set_coefficients(_lane(i, gain, pre, 2000 + 10 * P + i), A)
        if kind == "loud":
            lane.gain = LOUD_GAINS[k % 3]
        C.memmove(C.byref(lanes[i]), C.byref(lane), C.sizeof(vs.Lane))
    return kinds, lanes


@functools.lru_cache(maxsize=None)
def hcase(name):
    """the batch "h22" (mixed pre-emphasis), "h22p1" (every lane at pre-emphasis 1, which selects the fused kernels'
    instantiation for that case) or "h40" """
    assert name in CASES
    P = 40 if name == "h40" else 22
    kinds, proto = _lanes(P)
    lanes = (vs.Lane * BATCH)()
    C.memmove(lanes, proto, C.sizeof(lanes))
    if name == "h22p1":
        for l in lanes:
            l.pre_emphasis = 1.0
    flow = pyoracle.source(lanes, NS)
    A, gain, pre, order = lane_sets(lanes, P)
    o, f = {}, {}
    o["exact"], y = ar.exact_unrounded(flow, A, gain, pre, order)
    f["exact"] = ar.first_nonfinite(y)
    o["fma"], y = ar.fma_state(flow, A, gain, pre, P)
    f["fma"] = ar.first_nonfinite(y)
    smallest = None
    if P == 22:
        o["f32"], y, small = ar.f32_state(flow, A, gain, pre)
        f["f32"] = ar.first_nonfinite(y)
        smallest = small.rows
    exact = pyoracle.filter(lanes, flow)
    for a in [flow, A, exact, kinds] + list(o.values()) + list(f.values()):
        a.setflags(write=False)
    return Case(name=name, lanes=lanes, kinds=kinds, P=P, flow=flow, A=A, gain=gain, pre=pre, order=order, o=o, f=f,
                exact=exact, f32_smallest=smallest)


def compared(f, ns):
    """bool [rows][ns]: the samples a row is compared on, n <= f"""
    return np.arange(ns)[None, :] <= np.asarray(f)[:, None]


# ---- the restatements ------------------------------------------------------------------------------------------------

def test_lane_sets_of_41_coefficients():
    """the generalised lane_sets is tests/test_arith_ref.py's at P = 22, the same with zeros behind it at P = 40, and
    the lane's own taps with zeros above its order for sets of up to 40 taps"""
    c = cases.batch(False)
    A22, gain, pre = cases.lane_sets(c.lanes)
    for P in (22, 40):
        A, g, p, order = lane_sets(c.lanes, P)
        assert A.shape == (len(c.lanes), P + 1) and np.array_equal(A[:, :23], A22) and not A[:, 23:].any()
        assert np.array_equal(g, gain) and np.array_equal(p, pre) and (order <= 22).all()
    h = hcase("h40")
    assert h.A.shape == (BATCH, 41) and sorted(set(h.order)) == sorted(set(ORDERS[40]) | set(UNSTABLE_ORDERS[40]))
    for i, l in enumerate(h.lanes):
        assert np.array_equal(h.A[i, :l.order + 1], l.A[:l.order + 1]) and not h.A[i, l.order + 1:].any()
    with pytest.raises(AssertionError):
        lane_sets(h.lanes, 22)


@pytest.mark.parametrize("name", CASES)
def test_the_exact_restatement_is_the_oracle(name):
    """vowel_new.c:266-289 restated in numpy, behind round2int, against the compiled oracle: bit for bit on every row
    and sample, behind a state that is not finite too (both loop over the lane's own order)"""
    c = hcase(name)
    got = tr.round2int(c.o["exact"])
    assert np.array_equal(got, c.exact), np.argwhere(got != c.exact)[:8]
    print("%s: the exact restatement behind round2int equals the oracle on %d x %d samples (%d rows lose a finite state)" % (
        name, BATCH, NS, (c.f["exact"] < NS).sum()))


def test_the_40_tap_fma_form_is_the_track_restatement_with_one_set():
    c = hcase("h40")
    rows = np.zeros(BATCH, dtype=tr.ROW_DTYPE)
    rows["n_sets"], rows["hop"], rows["length"], rows["gain"], rows["pre_emphasis"] = 1, 1, NS, c.gain, c.pre
    want, _ = tr.filter_track(c.flow, c.A[:, None, :], rows, tr.HOLD, arith="fma")
    got, f = c.want("round2int")
    seen = compared(f, NS)                       # (behind f both are numpy's conversion of NaN: not compared)
    assert np.array_equal(got[seen], want[seen]) and np.abs(want.astype(np.int32)).max() == 32767


# ---- the conditions --------------------------------------------------------------------------------------------------

def saturated(pcm):
    return np.abs(pcm.astype(np.int32)) == 32767


def check_conditions(c):
    """the conditions under which a byte-for-byte comparison on this batch tells a right kernel from a wrong one;
    returns the lines for the profile"""
    lines = []
    lib = vs.load()
    P = c.P
    assert len(c.lanes) == BATCH and all(l.out_snr == 0.0 and l.vowel == 0 for l in c.lanes)
    assert all(lib.vs_lane_validate(C.byref(l)) == 0 for l in c.lanes)       # lanes a plan accepts
    assert all(l.pre_emphasis == 1.0 for l in c.lanes) == (c.name == "h22p1")
    assert set(c.order) <= set(ORDERS[P]) | set(UNSTABLE_ORDERS[P]) and set(c.order) >= set(ORDERS[P])
    assert (c.order.max() > 22) == (P == 40)     # one lane above 22 taps makes the plan wide
    for k in PREFIXES[:-1]:
        assert len(set(c.kinds[:k])) >= min(k, 4), (k, c.kinds[:k])
    ariths = ("exact", "fma") + (("f32",) if P == 22 else ())
    # loud lanes: the bands, per arithmetic
    loud = c.rows("loud")
    for name in ariths:
        o = c.o[name]
        assert np.isfinite(o[loud]).all() and (c.f[name][loud] == NS).all(), name
        peaks = []
        for g, (lo, hi) in zip(LOUD_GAINS, LOUD_BANDS):
            r = loud[c.gain[loud] == np.float32(g)]
            assert len(r) >= 12, (g, len(r))
            pk = np.abs(o[r]).max(axis=1)
            assert (pk > lo).all() and (pk < hi).all(), (name, g, pk.min(), pk.max())
            peaks.append("%.3g..%.3g at gain %g (%d rows)" % (pk.min(), pk.max(), g, len(r)))
        r1 = loud[c.gain[loud] == np.float32(LOUD_GAINS[0])]
        free = float((np.abs(o[r1]) < 32767.0).mean())
        assert 0.05 <= free <= 0.95, (name, free)
        lines.append("loud lanes, %s: max |o| per row %s; %.1f %% of the gain-%g samples unclamped" % (
            name, ", ".join(peaks), 100 * free, LOUD_GAINS[0]))
    # unstable lanes: the first state that is not finite lies in the window, in the arithmetic the lane is made for
    for kind, names in (("unstable", ("exact", "fma")), ("unstable32", ("f32",) if P == 22 else ())):
        u = c.rows(kind)
        # (the ragged group has two lanes: one is unstable in double, and with that in single precision too)
        assert len(u) >= 8 and (u < 64).any() and ((u >= 64) & (u < 128)).any() and ((u >= 128).any() or kind == "unstable32"), u
        for name in names:
            f = c.f[name][u]
            assert (f >= WINDOW[0]).all() and (f <= WINDOW[1]).all(), (kind, name, f)
            lines.append("%s lanes (%d rows, orders %s), %s: first state that is not finite at n = %d..%d" % (
                kind, len(u), sorted(int(v) for v in set(c.order[u])), name, f.min(), f.max()))
    assert set(c.order[c.rows("unstable")]) == {1} | set(UNSTABLE_ORDERS[P])
    for name in ariths:                          # nothing else loses its state (in double: nor the unstable32 lanes)
        lost = c.f[name] < NS
        allowed = (c.kinds == "unstable") | ((c.kinds == "unstable32") & (name == "f32"))
        assert not (lost & ~allowed).any(), (name, np.flatnonzero(lost & ~allowed))
    if P == 22:
        early = c.f["f32"][c.rows("unstable")]
        lines.append("unstable lanes in single precision: the state leaves float32 at n = %d..%d" % (early.min(), early.max()))
        assert (c.f32_smallest >= ar.F32_MIN_NORMAL).all(), c.f32_smallest.min()
        lines.append("smallest non-zero finite single-precision intermediate %.3e" % c.f32_smallest.min())
    # a stable lane of order 5 right behind every unstable lane of order 1
    u1 = np.array([r for r in c.rows("unstable") if c.order[r] == 1])
    assert len(u1) >= 4 and (c.kinds[u1 + 1] == "neighbour").all() and (c.order[u1 + 1] == 5).all()
    assert {float(c.A[r, 1]) for r in u1} == {4.0, -4.0}
    # tame lanes stay inside int16 mostly
    tame = np.concatenate([c.rows("tame"), c.rows("neighbour")])
    assert (c.gain[tame] >= 1).all() and (c.gain[tame] <= 10).all() and saturated(c.exact[tame]).mean() < 0.5
    # tie and split lanes
    r2i = c.want("round2int")[0]
    sp, tie = c.rows("split"), c.rows("tie")
    assert not c.A[tie, 1:].any() and (c.gain[tie] == TIE_GAIN).all() and (c.gain[sp] == TIE_GAIN).all()
    differs = r2i[sp] != c.exact[sp]
    assert differs.sum() >= 10 and differs.any(axis=1).sum() >= 3, (differs.sum(), differs.any(axis=1).sum())
    assert np.abs(r2i[sp].astype(np.int32) - c.exact[sp]).max() == 1 and not saturated(c.exact[sp]).any()
    lines.append("split-sum lanes (taps %s): FMA form differs from the exact oracle in %d of %d samples on %d of %d rows (by 1 LSB)" % (
        " ".join(str(t) for t in SPLIT_TAPS[P]), differs.sum(), differs.size, differs.any(axis=1).sum(), len(sp)))
    if P == 40:
        # the split taps sit above tap 22, and a form that stops short of tap 40 is another function on the rows that
        # carry the last taps
        assert all(min(t for t in range(3, 41) if c.A[r, t]) > 22 or c.A[r, 40] for r in sp)
        for tap in (39, 40):
            r = np.flatnonzero(c.A[:, tap] != 0.0)
            short = np.array(c.A[r])
            short[:, tap] = 0.0
            o, y = ar.fma_state(c.flow[r], short, c.gain[r], c.pre[r], 40)
            seen = compared(np.minimum(c.f["fma"][r], ar.first_nonfinite(y)), NS)
            d = (tr.round2int(o) != r2i[r]) & seen
            assert d.any(axis=1).sum() >= 3 and (tap == 39 or d[np.isin(r, sp)].any(axis=1).sum() >= 3), (tap, d.any(axis=1))
            lines.append("FMA form without tap %d: differs in %d samples on %d of the %d rows that carry it (%d of them split-sum rows)" % (
                tap, d.sum(), d.any(axis=1).sum(), len(r), d[np.isin(r, sp)].any(axis=1).sum()))
    if c.name != "h22p1":
        even, up = c.want("nearest_even")[0], c.want("half_up")[0]
        assert np.array_equal(c.o["fma"][tie], c.flow[tie] * TIE_GAIN)
        for name, d in (("round2int / nearest even", r2i[tie] != even[tie]), ("round2int / half up", r2i[tie] != up[tie])):
            assert d.mean() >= 0.10, (name, d.mean())
        lines.append("tie lanes: round2int and nearest-even differ in %.1f %% of the samples" % (100 * (r2i[tie] != even[tie]).mean()))
    return lines


@pytest.mark.parametrize("name", CASES)
def test_batch_conditions(name):
    for line in check_conditions(hcase(name)):
        print("%-5s: %s" % (name, line))


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_flow_of_a_shorter_call_is_a_prefix(name):
    """the expected bytes of every sample count are prefixes of the 1000-sample restatement: the flow must be one"""
    c = hcase(name)
    for ns in SAMPLE_COUNTS[c.P]:
        assert np.array_equal(pyoracle.source(c.lanes, ns), c.flow[:, :ns]), ns
