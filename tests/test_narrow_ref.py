"""The batches of the narrow build of the one-wave kernel (tests/test_gpu_narrow.py: csrc/vs_synth_one_wave.hip compiled with
VS_GROUP_LANES = 16 for periods beyond the 64-column ring) and the conditions under which a byte-for-byte comparison on
them means something, built and asserted on the CPU from the oracle and the restatements of tests/arith_ref.py, in the
style of tests/test_synth_hostile_ref.py.

  N22    33 lanes: two whole groups of 16 and a ragged group of one.  Every lane has source options of its own near the
         shortest periods that make a plan narrow (48 .. 64 kHz, F0 50 .. 55 Hz, cq 0.30 .. 0.89; 3 % jitter on three
         lanes of four, shimmer and glottal noise mixed, every eighth lane in the carried-T4 regime of
         tests/test_gpu_carried_t4.py), so that a group of 16 stages a cos row per lane and 4000 samples hold three
         cycles and more.  The filter kinds of tests/test_arith_ref.py are dealt through the batch by a pattern of 11:
         table lanes, explicit sets of orders 1, 2, 5, 12, 21 and 22, tie, split and saturating lanes.  No lane is unstable.
  N22p1  the same with every lane at pre-emphasis 1 (the exact kernel's instantiation for that case).
  N40    the same source lanes with sets of orders 1 .. 40 (lane 0 the widest): the wide filter kernel behind the narrow
         source kernel.
SHORT_LONG is the batch of tests/test_gpu_narrow.py part d: 48 lanes, one long-period lane among 15 short ones in every
16 of them (the plan's order, by period, gathers the three in its last wavefront).  REFUSED is the 15-lane batch a plan refuses although each of its lanes passes alone
(tests/c/test_planhost_asan.c holds the same lanes against the limit itself).  Every test prints a line per case."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi, configs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arith_ref as ar  # noqa: E402
import test_cycle_log_ref as logref  # noqa: E402
import test_synth_hostile_ref as hostile  # noqa: E402
from test_arith_ref import SPLIT_TAP, TABLE_GAINS, TABLE_PRES, TABLES, TIE_GAIN  # noqa: E402

NS = 4000
BATCH = 33                   # two whole groups of 16 utterances and a ragged one
GROUP = 16                   # utterances per wavefront of the narrow build
PREFIXES = (1, 15, 16, 17)
FEW = (25, NS)               # the sample counts of the prefixes
LOG_PITCHES = (4, 16)
ORDERS = {22: (1, 2, 5, 12, 21, 22), 40: hostile.ORDERS[40]}
CASES = ("n22", "n22p1", "n40")
PATTERN = ("set", "table", "tie", "split", "sat", "set", "table", "split", "set", "tie", "set")
assert BATCH % len(PATTERN) == 0
# the even taps of the split lanes; in N40 they sit above tap 22, three of them: 24 to 40 samples back a neighbour shares
# the binade of x * gain less often than two samples back, and three products pass half a last bit more often than two
SPLIT_TAPS = {22: hostile.SPLIT_TAPS[22], 40: ((24, 26, 28), (24, 32, 40), (30, 38, 40), (26, 34, 40))}
# the longest period the 64-column ring takes (vs_ring_policy_for: 1152 slots less a super-step and the trash rows): a
# batch with a lane whose rejection test admits a longer one runs on the narrow build
WIDE_RING_TBOUND = 1152 - 24 - 8
RATES = (64000, 56000, 48000, 50000)


def source_args(i):
    """flowgen_shimmer's options of lane i: rate, F0, cq, jitter, shimmer, glottal noise, DC flow and amplitude all
    change from lane to lane.  Lanes 0, 1 (mod 4) have periods of 1018 .. 1280 samples, the others 872 .. 1000.  The
    split lanes go without glottal noise and have the longest open phases (cq 0.90 .. 0.96): what tells the FMA form
    from the exact one there is a rounding tie in x * gain next to neighbours of the same binade, which a smooth flow
    has at every odd sample and a noisy one at a third of them"""
    fs = RATES[i % 4]
    f0 = 50.0 + 0.5 * ((7 * i) % 11)
    split = PATTERN[i % len(PATTERN)] == "split"
    cq = 0.90 + 0.002 * i if split else 0.30 + 0.59 * ((13 * i) % BATCH) / (BATCH - 1.0)
    fa = ["-r", str(fs), "-d", "0.5", "-f", "%.1f" % f0, "-g", "%.1f" % (f0 * 125.0 / 120.0 + 1.0), "-c", "%.4f" % cq]
    if i % 4 != 3:
        fa += ["-j", "3"]
    if i % 8 == 4:                               # zero DC flow, an amplitude shimmer takes past 32767, noise
        fa += ["-l", "0", "-a", str(27000 + 500 * (i // 8)), "-s", "%.2f" % (12.0 + i), "-n", "%.1f" % (8.0 + i)]
    else:
        if i % 3 != 0:
            fa += ["-s", "%.2f" % (2.0 + 0.5 * i)]
        if i % 2 == 1 and not split:
            fa += ["-n", "%.1f" % (5.0 + i)]
        if i % 5 == 2:
            fa += ["-k", "%.2f" % (0.5 + 0.02 * i), "-z", "%.2f" % (0.01 * i)]
    return fa


def expand(lane):
    """the record the kernels read of a lane (csrc/vs_planhost.c, vs_expand_lane)"""
    d = _ffi.DevLane()
    vs.check(vs.load().vs_expand_lane(C.byref(lane), 0, C.byref(d)), "vs_expand_lane")
    return d


def kernel_order(lanes):
    """the order a plan puts its records in: stable by (P, T2, jitter / shimmer / noise on) (vs_expand_all_ordered)"""
    recs = [expand(l) for l in lanes]
    return sorted(range(len(recs)), key=lambda i: (recs[i].P, recs[i].T2, recs[i].flags & 7)), recs


def group_rows(lanes):
    """per wavefront of the narrow build: (distinct T2, cos-row entries (T2 + 7) & ~7 summed over them, longest tbound)"""
    order, recs = kernel_order(lanes)
    out = []
    for g in range(0, len(order), GROUP):
        t2 = sorted({recs[i].T2 for i in order[g:g + GROUP]})
        out.append((len(t2), sum((t + 7) & ~7 for t in t2), max(recs[i].tbound for i in order[g:g + GROUP])))
    return out


class Case(dict):
    """one batch and what the oracle and the restatements make of it: lanes, kinds, P, flow (the oracle's, read-only), A /
    gain / pre / order, exact (the oracle's PCM), o_fma (the FMA form over P taps before its rounding), y_exact / y_fma
    (the states)"""
    __getattr__ = dict.__getitem__

    def rows(self, kind):
        return np.flatnonzero(self.kinds == kind)

    def want(self, family, lanes=BATCH, ns=NS):
        """int16 [lanes][ns]: "exact" or one of ar.ROUNDINGS (the FMA form behind it)"""
        if family == "exact":
            return self.exact[:lanes, :ns]
        return ar.rounded(self.o_fma[:lanes, :ns], family)


@functools.lru_cache(maxsize=None)
def _lanes(P):
    """(kinds, lanes) of the mixed pre-emphasis variant"""
    rng = np.random.default_rng(1600 + P)
    kinds = np.array([PATTERN[i % len(PATTERN)] for i in range(BATCH)])
    lanes = (vs.Lane * BATCH)()
    count = {k: 0 for k in set(PATTERN)}
    for i, kind in enumerate(kinds):
        k = count[kind]
        count[kind] += 1
        A = None
        if kind == "table":
            va = ["-v", TABLES[(3 * k + 1) % 10], "-g", TABLE_GAINS[k % 3], "-p", TABLE_PRES[k % 4]]
        elif kind == "sat":
            va = ["-v", TABLES[(7 * k) % 10], "-g", "30" if k % 3 == 2 else "1000", "-p", TABLE_PRES[(k + 1) % 4]]
        elif kind == "set":
            order = ORDERS[P][(k - 1) % len(ORDERS[P])]          # (lane 0 has the most taps: every prefix of N40 is wide)
            A = configs.random_pole_set(order, rng)
            va = ["-v", "a", "-g", "%.2f" % rng.uniform(1, 10), "-p", TABLE_PRES[i % 4]]
        else:
            va = ["-v", "a", "-g", "%g" % TIE_GAIN, "-p", "0"]
            A = np.concatenate([[1.0], np.zeros(P)])
            if kind == "split":
                A[list(SPLIT_TAPS[P][k % len(SPLIT_TAPS[P])])] = SPLIT_TAP
        lane = vs.lane_from_cli(source_args(i), va, 1600 + 10 * P + i)[0]
        if A is not None:
            lane = vs.set_coefficients(lane, A)
        C.memmove(C.byref(lanes[i]), C.byref(lane), C.sizeof(vs.Lane))
    return kinds, lanes


@functools.lru_cache(maxsize=None)
def ncase(name):
    """the batch "n22" (mixed pre-emphasis), "n22p1" (every lane at pre-emphasis 1) or "n40" """
    assert name in CASES
    P = 40 if name == "n40" else 22
    kinds, proto = _lanes(P)
    lanes = (vs.Lane * BATCH)()
    C.memmove(lanes, proto, C.sizeof(lanes))
    if name == "n22p1":
        for l in lanes:
            l.pre_emphasis = 1.0
    flow = po.source(lanes, NS)
    A, gain, pre, order = hostile.lane_sets(lanes, P)
    o_exact, y_exact = ar.exact_unrounded(flow, A, gain, pre, order)
    o_fma, y_fma = ar.fma_state(flow, A, gain, pre, P)      # (a Python loop over the samples: once per case)
    exact = po.filter(lanes, flow)
    for a in (flow, A, exact, kinds, o_exact, o_fma, y_exact, y_fma):
        a.setflags(write=False)
    return Case(name=name, lanes=lanes, kinds=kinds, P=P, flow=flow, A=A, gain=gain, pre=pre, order=order, exact=exact,
                o_exact=o_exact, o_fma=o_fma, y_exact=y_exact, y_fma=y_fma)


@functools.lru_cache(maxsize=None)
def first_periods():
    """the first cycle of every lane of N22 (the oracle's log)"""
    recs, ncyc, _ = logref.oracle_log(ncase("n22").lanes, NS, 1)
    return np.array(recs["T"][:, 0])


def sample_counts():
    """around the super-step of 24, one count below the shortest first period of the batch (no lane finishes a cycle),
    an odd count and the whole"""
    return (1, 23, 24, 25, int(first_periods().min()) - 1, NS - 1, NS)


def shapes():
    """(lanes, samples) of every launch of a grid point: the whole batch at every sample count, the prefixes at two"""
    return [(BATCH, ns) for ns in sample_counts()] + [(k, ns) for k in PREFIXES for ns in FEW]


@functools.lru_cache(maxsize=None)
def log_of(name, pitch):
    """(records [33][pitch], ncyc) of a 4000-sample run: every lane's own vs_oracle_source"""
    recs, ncyc, _ = logref.oracle_log(ncase(name).lanes, NS, pitch)
    return recs, ncyc


# ---- part d: one long lane among short ones --------------------------------------------------------------------------

SHORT_LONG = 48


@functools.lru_cache(maxsize=None)
def short_long_lanes():
    """48 lanes: the lanes at l % 16 == 5 have N22's source options of lanes 0, 4 and 8 (periods beyond the 64-column
    ring), the others run at 16000 and 22050 Hz with F0 100 .. 250 (the generator's short sequences among them)"""
    c = ncase("n22")
    lanes = (vs.Lane * SHORT_LONG)()
    for l in range(SHORT_LONG):
        if l % GROUP == 5:
            src = c.lanes[4 * (l // GROUP)]
        else:
            fs = (16000, 22050)[l % 2]
            f0 = 100.0 + 150.0 * ((11 * l) % SHORT_LONG) / (SHORT_LONG - 1.0)
            # (22050 Hz is the rate of a command line without -r: the reference refuses it when it is spelt out)
            fa = (["-r", str(fs)] if fs != 22050 else []) + ["-d", "0.5", "-f", "%.1f" % f0, "-g", "%.1f" % (f0 * 125.0 / 120.0 + 1.0)]
            if l % 3:
                fa += ["-j", "1", "-s", "5.76", "-n", "20"]
            src = vs.lane_from_cli(fa, ["-v", TABLES[l % 10], "-g", TABLE_GAINS[l % 3], "-p", TABLE_PRES[l % 4]], 4800 + l)[0]
        C.memmove(C.byref(lanes[l]), C.byref(src), C.sizeof(vs.Lane))
    return lanes


# ---- part i: the batch a plan refuses --------------------------------------------------------------------------------

# (fs, F0, Fg, cq) of tests/c/test_planhost_asan.c, refused_lanes: periods near the top of the narrow build's range and a
# cos row of its own per lane.  Every other field is vs_lane_defaults'
REFUSED = ((176400, 50.0, 52.0, 0.30), (176400, 56.0, 58.0, 0.35), (176400, 64.0, 66.0, 0.42), (176400, 79.0, 81.0, 0.45),
           (96000, 50.0, 52.0, 0.55), (96000, 52.0, 54.0, 0.60), (96000, 55.0, 57.0, 0.65), (96000, 60.0, 62.0, 0.70),
           (88200, 50.0, 52.0, 0.75), (88200, 53.0, 55.0, 0.80), (88200, 58.0, 60.0, 0.85), (88200, 66.0, 68.0, 0.89),
           (44100, 50.0, 52.0, 0.85), (44100, 51.0, 53.0, 0.89), (44100, 79.0, 81.0, 0.80))


@functools.lru_cache(maxsize=None)
def refused_lanes():
    lanes = (vs.Lane * len(REFUSED))()
    for i, (fs, f0, fg, cq) in enumerate(REFUSED):
        lane = vs.default_lane()
        lane.fs, lane.F0, lane.Fg, lane.cq, lane.seed = fs, f0, fg, cq, 900 + i
        C.memmove(C.byref(lanes[i]), C.byref(lane), C.sizeof(vs.Lane))
    return lanes


# ---- the conditions --------------------------------------------------------------------------------------------------

def saturated(pcm):
    return np.abs(pcm.astype(np.int32)) == 32767


def check_conditions(c):
    """the conditions under which a byte-for-byte comparison on this batch tells a right narrow kernel from a wrong one;
    returns the lines for the profile"""
    lines = []
    lib = vs.load()
    P = c.P
    assert len(c.lanes) == BATCH and all(l.out_snr == 0.0 for l in c.lanes)
    assert all(lib.vs_lane_validate(C.byref(l)) == 0 for l in c.lanes)       # lanes a plan accepts
    assert all(l.pre_emphasis == 1.0 for l in c.lanes) == (c.name == "n22p1")
    assert (c.order.max() > 22) == (P == 40) and c.order[0] == P and set(c.order) >= set(ORDERS[P])
    # the source options: rate, F0 and cq differ, jitter / shimmer / noise are on and off, every launched prefix is narrow
    recs = [expand(l) for l in c.lanes]
    assert len({l.fs for l in c.lanes}) == 4 and len({l.F0 for l in c.lanes}) >= 10 and len({l.cq for l in c.lanes}) == BATCH
    for flag in (vs.VS_FLAG_JITTER, vs.VS_FLAG_SHIMMER, vs.VS_FLAG_NOISE):
        on = sum(1 for l in c.lanes if l.flags & flag)
        assert 8 <= on <= BATCH - 8, (flag, on)
    assert recs[0].tbound > WIDE_RING_TBOUND                                  # lane 0 lies in every prefix
    fast = [bool(r.flags & _ffi.VS_DF_FAST) for r in recs]
    assert any(fast) and not all(fast)
    carried = [i for i, l in enumerate(c.lanes) if l.DC == 0.0 and l.amp >= 24000 and l.flags & vs.VS_FLAG_NOISE
               and l.flags & vs.VS_FLAG_SHIMMER]
    assert len(carried) >= 4 and min(carried) < 15
    groups = group_rows(c.lanes)
    assert len(groups) == 3 and max(g[0] for g in groups) >= 12, groups
    for k in PREFIXES:
        assert len(set(c.kinds[:k])) >= min(k, 4), (k, c.kinds[:k])
        assert max(r.tbound for r in recs[:k]) > WIDE_RING_TBOUND
    lines.append("periods P %d..%d, tbound %d..%d, T2 %d..%d; per wavefront (distinct T2, cos-row entries, longest tbound) %s; "
                 "%d lanes on the short sequences, %d in the carried-T4 regime" % (
                     min(r.P for r in recs), max(r.P for r in recs), min(r.tbound for r in recs), max(r.tbound for r in recs),
                     min(r.T2 for r in recs), max(r.T2 for r in recs), groups, sum(fast), len(carried)))
    # no lane loses its state: every sample is compared
    for name, y in (("exact", c.y_exact), ("fma", c.y_fma)):
        assert np.isfinite(y).all() and np.isfinite(c[{"exact": "o_exact", "fma": "o_fma"}[name]]).all(), name
    # the exact restatement is the oracle, and the oracle's filter behind its source is its synthesis
    assert np.array_equal(ar.rounded(c.o_exact, "round2int"), c.exact)
    assert np.array_equal(po.synth(c.lanes, NS), c.exact)
    # the cycle counts of a 4000-sample run: three cycles and more, and no more than the longer log holds
    recs16, ncyc = log_of(c.name, LOG_PITCHES[1])
    assert ncyc.min() >= 3 and ncyc.max() <= LOG_PITCHES[1] and (ncyc > LOG_PITCHES[0]).any(), (ncyc.min(), ncyc.max())
    lines.append("cycles of %d samples: %d..%d per lane (log pitches %s)" % (NS, ncyc.min(), ncyc.max(), list(LOG_PITCHES)))
    # the split lanes tell the FMA form from the exact one, the tie lanes round2int from nearest-even
    r2i = c.want("round2int")
    sp, tie = c.rows("split"), c.rows("tie")
    assert len(sp) >= 4 and len(tie) >= 4
    differs = r2i[sp] != c.exact[sp]
    if c.name == "n22p1":
        # (pre-emphasis 1 takes the neighbour's state off again: a last bit of the state shows in the few samples whose
        # difference lands on a tie.  The floor of tests/test_synth_hostile_ref.py)
        assert differs.sum() >= 10 and differs.any(axis=1).sum() >= 3, (differs.sum(), differs.any(axis=1).sum())
    else:
        assert differs.mean() > 0.25 and differs.any(axis=1).all(), (differs.mean(), differs.mean(axis=1))
    assert np.abs(r2i[sp].astype(np.int32) - c.exact[sp]).max() == 1 and not saturated(c.exact[sp]).any()
    lines.append("split-sum lanes (taps %s): FMA form differs from the exact oracle in %d of %d samples (%.1f %%, by 1 LSB)" % (
        " ".join(str(t) for t in SPLIT_TAPS[P]), differs.sum(), differs.size, 100 * differs.mean()))
    if c.name != "n22p1":
        even = c.want("nearest_even")
        assert not c.A[tie, 1:].any() and (c.gain[tie] == TIE_GAIN).all() and (c.pre[tie] == 0.0).all()
        d = r2i[tie] != even[tie]
        assert d.mean() >= 0.10 and d.any(axis=1).all(), (d.mean(), d.mean(axis=1))
        lines.append("tie lanes: round2int and nearest-even differ in %.1f %% of the samples" % (100 * d.mean()))
    others = np.flatnonzero(c.kinds != "split")
    lines.append("every other lane: FMA form differs from the exact oracle in %d of %d samples" % (
        (r2i[others] != c.exact[others]).sum(), r2i[others].size))
    sat = saturated(c.exact[c.rows("sat")])
    # (behind pre-emphasis 1 the gain-30 lane stays inside int16 at these periods)
    assert sat.any(axis=1).sum() >= (2 if c.name == "n22p1" else 3) and not sat.all(axis=1).any(), sat.mean(axis=1)
    lines.append("saturating lanes: %.1f %% of the samples at the clamp" % (100 * sat.mean()))
    return lines


@pytest.mark.parametrize("name", CASES)
def test_batch_conditions(name):
    for line in check_conditions(ncase(name)):
        print("%-5s: %s" % (name, line))


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_flow_and_log_of_a_shorter_call_are_prefixes(name):
    """the expected bytes of every sample count are prefixes of the 4000-sample restatement: the flow must be one.  The
    shortest count lies inside every lane's first cycle"""
    c = ncase(name)
    counts = sample_counts()
    assert counts[4] < first_periods().min() and counts[4] > 25 and len(set(counts)) == 7
    for ns in counts:
        assert np.array_equal(po.source(c.lanes, ns), c.flow[:, :ns]), ns
    print("%s: sample counts %s; first periods %d..%d" % (name, list(counts), first_periods().min(), first_periods().max()))


def test_one_long_lane_among_short_ones():
    lanes = short_long_lanes()
    order, recs = kernel_order(lanes)
    long_ones = [l for l in range(SHORT_LONG) if recs[l].tbound > WIDE_RING_TBOUND]
    assert long_ones == [5, 21, 37]
    short = [recs[l] for l in range(SHORT_LONG) if l % GROUP != 5]
    assert max(r.tbound for r in short) < 300 and {l.fs for l in lanes} >= {16000, 22050}
    assert any(r.flags & _ffi.VS_DF_FAST for r in short)
    groups = group_rows(lanes)
    print("short and long: 45 lanes of tbound %d..%d and 3 of %s; per wavefront in kernel order (distinct T2, cos-row "
          "entries, longest tbound) %s" % (min(r.tbound for r in short), max(r.tbound for r in short),
                                          [recs[l].tbound for l in long_ones], groups))
    assert len(groups) == 3 and groups[-1][2] > WIDE_RING_TBOUND


def test_every_lane_of_the_refused_batch_passes_alone():
    """what a plan needs of its worst wavefront -- the smallest ring (a super-step, the longest cycle, the trash rows, up
    to a multiple of the super-step) of 16 columns and the cos rows of its distinct T2 -- passes a compute unit's LDS for
    the 15 lanes together and stays inside it for each of them alone"""
    lanes = refused_lanes()
    lds_limit, ss, trash = 160 * 1024, 24, 8
    need = lambda tb, entries: ((ss + tb + trash + ss - 1) // ss * ss + trash) * GROUP * 2 + entries * 8      # noqa: E731
    (n_t2, entries, tb), = group_rows(lanes)
    assert n_t2 == len(lanes) == 15 and need(tb, entries) > lds_limit, (n_t2, entries, tb)
    alone = [group_rows([l])[0] for l in lanes]
    assert all(need(t, e) <= lds_limit for _, e, t in alone)
    print("refused batch: longest tbound %d, %d cos-row entries over %d distinct T2: %d bytes of LDS; alone the lanes need "
          "%d..%d bytes (limit %d)" % (tb, entries, n_t2, need(tb, entries), min(need(t, e) for _, e, t in alone),
                                       max(need(t, e) for _, e, t in alone), lds_limit))
