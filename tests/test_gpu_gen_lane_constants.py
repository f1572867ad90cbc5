"""The generator's lane-constant shortcuts on the device, sample for sample against the oracle, in every kernel family a
tuning can steer a plan to (three roles role-major, three roles in the spread layout, two roles, the one-wave kernel)
and in VS_ARITH_EXACT and VS_ARITH_FMA:

  - a group whose valid lanes share T2 and K, with Kvar == 0 and the short sequences, stages its falling-flank row
    instead of the cos row and reads the rising flank's cos values with scalar loads (csrc/vs_dev_generator.h, "A UNIFORM
    group"):
    T2 a multiple of 8 and not, batches of 65 and 100 utterances (the last group partly filled: uniform over its valid
    lanes only);
  - groups that are NOT uniform keep the cos rows: Kvar == 0 next to Kvar == 0.3 (the closing-speed draw is skipped only
    where no lane of the wavefront needs it), two K at one T2, two T2, and a group uniform but for one lane that is not
    VS_DF_FAST (the general sequences read the cos row);
  - DC > 0 with and without glottal noise: the below-DC and the break trips of both flanks;
  - amplitudes 50 .. 32000 and noise 0 .. 50 dB (the range vs_lane_validate admits) in one batch: noise widths from 0 to
    above VS_NDW_FAST through the integer square root (the oracle's log bounds each width from both sides: some are 0,
    some lie above 65534); the cycle log is compared with the oracle's as well;
  - the largest jitter and shimmer vs_lane_validate admits, at F0 = 80 and 300 Hz: the rejection loops iterate, the
    draw counts (the cycle counts of every family, and the log's T) are the oracle's.

The PCM is oracle.pyoracle.synth's in both arithmetics: the source does not depend on the arithmetic, and the lanes'
filter (table a at gain 2) is one on which the FMA forms (tests/arith_ref.py) give the exact form's bytes on these flows --
a case on which they did not would fail here in VS_ARITH_FMA alone, and would have to go.  Every case is at most 256
utterances x 4000 samples; the oracle's answers are computed once per case."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cycle_log_ref as logref  # noqa: E402
from test_cycle_log_ref import as_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4000
VS_DF_FAST = 8
CANARY32 = 0x5A5A5A5A
# (tuning, roles -- 0: the one-wave kernel --, layout); rings of 240 slots so that four groups share a workgroup
FAMILIES = {
    "three-roles-role-major": (dict(kernel=vs.VS_KERNEL_WS, ws_roles=3, ws_pairs=4, ring_slots=240), 3, "role-major"),
    "three-roles-spread": (dict(kernel=vs.VS_KERNEL_WS, ws_roles=3, ws_pairs=2, ring_slots=240), 3, "spread"),
    "two-roles": (dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ws_pairs=1), 2, "role-major"),
    "one-wave": (dict(kernel=vs.VS_KERNEL_SINGLE), 0, None),
}
ARITHS = {"exact": vs.VS_ARITH_EXACT, "fma": vs.VS_ARITH_FMA}
BASE = ["-r", "16000", "-d", "0.5", "-j", "1", "-s", "5.76", "-n", "20"]     # BASELINE config 3's command line: P = 133, T2 = 37


def _lanes(n, fa_of, va=("-v", "a", "-g", "2")):
    arr = (vs.Lane * n)()
    for i in range(n):
        lane, _ = vs.lane_from_cli(fa_of(i), list(va), 9000 + 7 * i)
        C.memmove(C.byref(arr[i]), C.byref(lane), C.sizeof(vs.Lane))
    return arr


def _records(lanes):
    out = []
    for lane in lanes:
        d = _ffi.DevLane()
        assert vs.load().vs_expand_lane(C.byref(lane), 0, C.byref(d)) == 0
        out.append((d.T2, d.K, d.Kvar, d.flags, d.P))
    return out


def _case_lanes(name):
    if name == "uniform-T2-37-100":
        return _lanes(100, lambda i: BASE)
    if name == "uniform-T2-40-65":
        return _lanes(65, lambda i: BASE + ["-c", "0.6"])
    if name == "mixed-Kvar":
        return _lanes(130, lambda i: BASE + ["-z", "0.3" if i % 2 else "0"])
    if name == "two-K":
        return _lanes(100, lambda i: BASE + ["-k", "0.8" if i % 3 == 0 else "0.65"])
    if name == "two-T2":
        return _lanes(100, lambda i: BASE + (["-c", "0.6"] if i % 2 else []))
    if name == "one-slow-lane":
        return _lanes(70, lambda i: BASE + (["-a", "32766"] if i == 5 else []))
    if name == "DC-with-noise":
        return _lanes(65, lambda i: BASE + ["-l", "0.2"])
    if name == "DC-without-noise":
        return _lanes(65, lambda i: ["-r", "16000", "-d", "0.5", "-j", "1", "-s", "5.76", "-l", "0.2"])
    if name == "widths":
        amps = [50, 200, 1000, 5000, 12000, 18000]           # with shimmer: (float)1.8*amp <= 32767, the short sequences
        lanes = _lanes(128, lambda i: BASE + ["-a", str(amps[i % 6])])
        loud = _lanes(128, lambda i: ["-r", "16000", "-d", "0.5", "-j", "1", "-n", "20", "-a", str((20000, 32000)[i % 2])])
        arr = (vs.Lane * 256)()
        for i in range(256):
            C.memmove(C.byref(arr[i]), C.byref((lanes if i < 128 else loud)[i % 128]), C.sizeof(vs.Lane))
            arr[i].noise = float(10.0 ** (((i * 7) % 51) / 10.0))      # 0 .. 50 dB, as flowgen_shimmer.c:511 stores it
        return arr
    if name in ("rejection-80Hz", "rejection-300Hz"):
        f0 = ["-g", "310", "-f", "300"] if name == "rejection-300Hz" else ["-g", "85", "-f", "80"]
        return _lanes(65, lambda i: ["-r", "16000", "-d", "0.5", "-j", "1000", "-s", "100", "-n", "20"] + f0)
    raise KeyError(name)


CASES = ["uniform-T2-37-100", "uniform-T2-40-65", "mixed-Kvar", "two-K", "two-T2", "one-slow-lane", "DC-with-noise",
         "DC-without-noise", "widths", "rejection-80Hz", "rejection-300Hz"]
RUNS = [(c, f) for c in CASES for f in sorted(FAMILIES)]      # every case in every family


@functools.lru_cache(maxsize=None)
def _case(name):
    """(lanes, records, oracle PCM, oracle log [lanes][400], ncyc)"""
    lanes = _case_lanes(name)
    recs = _records(lanes)
    pcm = po.synth(lanes, N)
    log, ncyc, _ = logref.oracle_log(lanes, N, 400)
    pcm.setflags(write=False)
    return lanes, recs, pcm, log, ncyc


def test_the_cases_are_what_they_are_meant_to_be():
    """from the records vs_expand_lane makes of them (no device work)"""
    def groups(recs):      # (the plan keeps the order of lanes whose P, T2 and options agree, and sorts the others by them)
        return [recs[i:i + 64] for i in range(0, len(recs), 64)]

    def uniform(g):
        return len({(t2, k) for t2, k, _, _, _ in g}) == 1 and all(kv == 0.0 and (f & VS_DF_FAST) for _, _, kv, f, _ in g)

    for name, t2 in (("uniform-T2-37-100", 37), ("uniform-T2-40-65", 40), ("DC-with-noise", 37), ("DC-without-noise", 37)):
        recs = _case(name)[1]
        assert all(uniform(g) for g in groups(recs)) and recs[0][0] == t2, name
        assert len(recs) % 64 != 0                                   # a partly filled last group
    assert 37 % 8 != 0 and 40 % 8 == 0
    recs = _case("mixed-Kvar")[1]
    assert {r[2] for r in recs[:64]} == {0.0, float(np.float32(0.3))} and len({(r[0], r[1]) for r in recs}) == 1
    recs = _case("two-K")[1]
    assert len({r[1] for r in recs[:64]}) == 2 and len({r[0] for r in recs}) == 1
    assert len({r[0] for r in _case("two-T2")[1]}) == 2
    recs = _case("one-slow-lane")[1]
    assert [i for i, r in enumerate(recs) if not r[3] & VS_DF_FAST] == [5] and len({(r[0], r[1], r[2]) for r in recs}) == 1
    for name in ("DC-with-noise", "DC-without-noise"):
        lanes = _case(name)[0]
        assert all(l.DC > 0 for l in lanes)
        assert all(bool(l.flags & vs.VS_FLAG_NOISE) == (name == "DC-with-noise") for l in lanes)
    lanes, recs, _, log, ncyc = _case("widths")
    live = np.arange(log.shape[1])[None, :] < ncyc[:, None]
    noise = np.array([l.noise for l in lanes])[:, None]
    # the width is (int)sqrt(12 * aux * x_pow / noise) with 1 <= aux = 1 + (T3 - T4) / T <= 2: between the floor and its sqrt(2)-fold
    width_floor = np.sqrt(12.0 * log["x_pow"].astype(np.float64) / noise)
    assert (width_floor[live] > 65534).any() and (width_floor[live] * np.sqrt(2.0) < 1.0).any()     # beyond VS_NDW_FAST, and 0
    assert all(r[3] & VS_DF_FAST for r in recs)
    assert min(l.amp for l in lanes) == 50 and max(l.amp for l in lanes) == 32000
    assert min(l.noise for l in lanes) == 1.0 and max(l.noise for l in lanes) == 100000.0
    for name, period in (("rejection-80Hz", 200), ("rejection-300Hz", 53)):
        lanes, recs, _, log, ncyc = _case(name)
        assert all(l.jitter == 10.0 and l.shimmer == 1.0 for l in lanes) and {r[4] for r in recs} == {period}
        # the loops iterate: more draws than the three per cycle and one per noise sample (at most one per sample)
        ndraws = logref.oracle_log(lanes, N, 1)[2]
        assert (ndraws > 3 * ncyc.astype(np.uint64) + N).sum() >= len(lanes) // 2, (ndraws[:8], ncyc[:8])


def _launch(eng, plan, nl, with_counts=True):
    with eng.scope() as dev:
        out_d = dev.filled((nl + 1) * N, 0x5A5A, np.int16)
        cnt_d = dev.filled(nl + 1, CANARY32, np.int32)
        plan.launch(vs.VS_KIND_SYNTH, out_d, ncyc_ptr=cnt_d)
        eng.synchronize()
        assert plan.status() == 0
        out = dev.get(out_d, (nl + 1, N))
        cnt = dev.get(cnt_d, (nl + 1,), np.int32)
    assert (out[nl] == 0x5A5A).all() and cnt[nl] == CANARY32
    return out[:nl], cnt[:nl]


@pytest.mark.parametrize("arith", sorted(ARITHS))
@pytest.mark.parametrize("name,family", RUNS)
def test_samples_and_cycle_counts_equal_the_oracle(name, family, arith):
    lanes, recs, pcm, log, ncyc = _case(name)
    tuning, roles, layout = FAMILIES[family]
    nl = len(lanes)
    with vs.Engine(0, arith=ARITHS[arith]) as eng:
        eng.set_tuning(**tuning)
        with eng.plan(lanes, N) as plan:
            kname = plan.kernel_name(vs.VS_KIND_SYNTH)
            pre1 = all(l.pre_emphasis == 1.0 for l in lanes)       # (the instantiation without the pre-emphasis product)
            if roles:
                assert kname == "vs_synth_ws_kernel<%d, %s, %d>" % (ARITHS[arith], "true" if pre1 else "false", roles), kname
                assert plan.roles()["roles"] == roles and plan.roles()["layout"] == layout, plan.roles()
            else:
                assert kname == "vs_synth_kernel<%d, 0, false, %s>" % (ARITHS[arith], "true" if pre1 and arith == "exact" else "false"), kname
            got, cnt = _launch(eng, plan, nl)
    want = pcm
    bad = (got != want).any(axis=1)
    print("%s, %s, %s: %s, %d lanes x %d samples, %d rows differ; cycle counts %d..%d, %d differ" % (
        name, family, arith, kname, nl, N, int(bad.sum()), int(ncyc.min()), int(ncyc.max()), int((cnt != ncyc).sum())))
    assert not bad.any(), (np.flatnonzero(bad)[:8], np.argwhere(got != want)[:4])
    assert np.array_equal(cnt, ncyc), np.flatnonzero(cnt != ncyc)[:8]


@pytest.mark.parametrize("name", ["widths", "rejection-80Hz", "rejection-300Hz", "DC-with-noise"])
def test_cycle_log_equals_the_oracle(name):
    """the kernels that keep a log (one-wave, LOG = true: the cos rows and the general sequences, and the square root)"""
    lanes, recs, pcm, log, ncyc = _case(name)
    with vs.Engine(0) as eng:
        flow, got_log, got_ncyc = eng.source(lanes, N, log_cycles=400)
    assert np.array_equal(got_ncyc, ncyc)
    assert np.array_equal(flow, po.source(lanes, N))
    bad = (as_bytes(got_log) != as_bytes(log)).any(axis=2)
    print("%s: %d records of %d lanes, %d differ; T %d..%d" % (name, int(ncyc.sum()), len(lanes), int(bad.sum()),
                                                             int(log["T"][log["T"] > 0].min()), int(log["T"].max())))
    assert not bad.any(), np.argwhere(bad)[:6]
