"""The narrow build of the one-wave kernel (csrc/vs_synth_one_wave.hip compiled with VS_GROUP_LANES = 16: periods beyond the
64-column ring), byte for byte against the oracle and the forms of include/voice_synth.h on every path a plan can send it
down:

  a. the instantiations <ARITH, KIND, false, PRE1>: synth, filter-only and source-only kind in the three contexts (the
     oracle in VS_ARITH_EXACT, the FMA form behind round2int in VS_ARITH_FMA and VS_ARITH_F32);
  b. ... and <ARITH, KIND, true, PRE1>: the cycle log and the counts, which do not depend on the arithmetic;
  c. shallow rings (vs_tuning.ring_slots: barely one cycle, 1.39 and 1.55 cycles) under every super-step threshold;
  d. one long-period lane among 15 short ones in every 16 lanes of a batch;
  e. layouts: pitches of n + 8, n + 2, n + 1 and n + 3, an odd length, bases 2 bytes off, an input pitch of its own;
  f. vowel -n's two passes behind it;   g. the wide filter kernel behind its source-only kind (sets of 23 .. 40 taps);
  h. the host calls, a long-period lane in the second chunk of the host pipeline, and a chunk of 4200 lanes whose rings hold
     barely one cycle;
  i. the batch a plan refuses although each of its lanes passes alone.

The batches and the conditions under which they mean something are built and asserted on the CPU in
tests/test_narrow_ref.py.  Every launch asserts that its plan is narrow, runs into sentinel-filled memory and leaves
vs_plan_status() == 0.  Every test prints what it compared (pytest -s): profiles/narrow_build.txt keeps those lines."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arith_ref as ar  # noqa: E402
import test_narrow_ref as cases  # noqa: E402
import test_synth_hostile_ref as hostile  # noqa: E402
from test_narrow_ref import BATCH, GROUP, LOG_PITCHES, NS, PREFIXES  # noqa: E402
from gpu_support import INPUT_PAD, SENTINEL, guarded_plan_launch, same_rows  # noqa: E402
from test_gpu_cycle_log import _canary_launch, _want  # noqa: E402
from test_gpu_cycle_log import _held as _log_held  # noqa: E402

pytestmark = pytest.mark.gpu

ARITHS = (vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA, vs.VS_ARITH_F32)
ARITH_NAME = {vs.VS_ARITH_EXACT: "EXACT", vs.VS_ARITH_FMA: "FMA", vs.VS_ARITH_F32: "F32"}
# the form the one-wave kernel runs in each context (the pairing of tests/test_gpu_arith.py)
FAMILY = {vs.VS_ARITH_EXACT: "exact", vs.VS_ARITH_FMA: "round2int", vs.VS_ARITH_F32: "round2int"}
FAMILY_TEXT = {"exact": "the oracle", "round2int": "the FMA form behind round2int"}
REMARK = " (narrow build: 16 utterances per wavefront)"
KIND_NAME = {vs.VS_KIND_SOURCE: "SOURCE", vs.VS_KIND_SYNTH: "SYNTH", vs.VS_KIND_FILTER: "FILTER"}


def _one(arith):
    """the arithmetic of the one-wave kernel's filter in a context"""
    return vs.VS_ARITH_FMA if arith == vs.VS_ARITH_F32 else arith


def _names(arith, lanes):
    """the kernel of each kind for these lanes in a context of that arithmetic (csrc/vs_planhost.c, pick_one_wave): only
    the exact filter has an instantiation for pre-emphasis 1, the source-only kind has no arithmetic to choose"""
    pre1 = "true" if _one(arith) == vs.VS_ARITH_EXACT and all(l.pre_emphasis == 1.0 for l in lanes) else "false"
    return {vs.VS_KIND_SYNTH: "vs_synth_kernel<%d, 0, false, %s>%s" % (_one(arith), pre1, REMARK),
            vs.VS_KIND_FILTER: "vs_synth_kernel<%d, 2, false, %s>%s" % (_one(arith), pre1, REMARK),
            vs.VS_KIND_SOURCE: "vs_synth_kernel<0, 1, false, false>%s" % REMARK}


def _narrow(name, info, n_lanes, want_name=None):
    """the plan of a launch is narrow: a wavefront per 16 utterances, and the remark behind the kernel's name"""
    assert info["workgroups"] == -(-n_lanes // GROUP), (name, info, n_lanes)
    assert REMARK in name, name
    if want_name is not None:
        assert name == want_name, (name, want_name)


def _launch(eng, lanes, ns, kind, want, what, want_name=None, **layout):
    """one guarded launch of a narrow plan against the rows it must give; returns (rows, name, info)"""
    got, name, info = guarded_plan_launch(eng, lanes, ns, kind, **layout)
    same_rows(got, want, (what, name, len(lanes), ns, layout))
    _narrow(name, info, len(lanes), want_name)
    return got, name, info


# a ---- the instantiations without a log

@pytest.mark.parametrize("arith", ARITHS)
def test_n22_synth_filter_and_source_kinds(arith):
    family = FAMILY[arith]
    with vs.Engine(0, arith=arith) as eng:
        for case in ("n22", "n22p1"):
            c = cases.ncase(case)
            seen, total = set(), 0
            for k, ns in cases.shapes():
                lanes, flow, want = c.lanes[:k], c.flow[:k, :ns], c.want(family, k, ns)
                names = _names(arith, lanes)
                _launch(eng, lanes, ns, vs.VS_KIND_SYNTH, want, case, names[vs.VS_KIND_SYNTH])
                _launch(eng, lanes, ns, vs.VS_KIND_FILTER, want, case, names[vs.VS_KIND_FILTER], flow=flow)
                _launch(eng, lanes, ns, vs.VS_KIND_SOURCE, flow, case, names[vs.VS_KIND_SOURCE])
                seen |= set(names.values())
                total += k * ns
            print("VS_ARITH_%s, %s: %d shapes %s, %d samples each: SYNTH and FILTER equal %s, SOURCE the oracle's flow; status 0, "
                  "guards and padding untouched; kernels %s" % (
                      ARITH_NAME[arith], case, len(cases.shapes()), cases.shapes(), total, FAMILY_TEXT[family],
                      sorted(n.replace(REMARK, "") for n in seen)))


# b ---- with the cycle log

@pytest.mark.parametrize("case", ["n22", "n22p1"])
def test_log_and_counts_in_the_exact_and_the_fma_context(case):
    c = cases.ncase(case)
    logs = {}
    for arith in (vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA):
        with vs.Engine(0, arith=arith) as eng:
            total, kernels = 0, set()
            for k in (BATCH,) + PREFIXES[1:]:
                lanes = c.lanes[:k]
                with eng.plan(lanes, NS) as plan:
                    names = _names(arith, lanes)
                    for kind, want_out in ((vs.VS_KIND_SOURCE, c.flow[:k]), (vs.VS_KIND_SYNTH, c.want(FAMILY[arith], k))):
                        _narrow(plan.kernel_name(kind), plan.info(), k, names[kind])
                        for pitch in LOG_PITCHES:
                            recs, ncyc = cases.log_of(case, pitch)
                            out, log, cnt = _canary_launch(eng, plan, k, NS, kind, pitch)
                            total += _log_held(out, log, cnt, want_out, recs[:k], ncyc[:k], pitch,
                                               (case, KIND_NAME[kind], ARITH_NAME[arith], k, pitch))
                            first = logs.setdefault((k, pitch), log)
                            assert np.array_equal(log, first), (k, pitch, KIND_NAME[kind], ARITH_NAME[arith])
                        # (a launch with a log takes LOG = true of the plan's kernel: csrc/vs_planhost.c, pick_one_wave)
                        kernels.add(names[kind].replace(REMARK, "").replace("false, ", "true, ", 1))
            print("with a log, VS_ARITH_%s, %s: %d lanes and the prefixes %s, SOURCE and SYNTH at log pitches %s: %d records "
                  "(canaries behind them), the counts (%d..%d) and the rows equal the oracle%s; one log in both kinds and "
                  "contexts; kernels %s" % (
                      ARITH_NAME[arith], case, BATCH, list(PREFIXES[1:]), list(LOG_PITCHES), total, ncyc.min(), ncyc.max(),
                      "" if arith == vs.VS_ARITH_EXACT else " (log, counts, flow) and the FMA form behind round2int (PCM)",
                      sorted(kernels)))


# c ---- rings

RING_DEPTHS = (0.0, 1.39, 1.55)      # cycles of the batch's longest period a ring holds behind its super-step; 0: the least
DEPTH_BANDS = {1.39: (1.33, 1.45), 1.55: (1.45, 1.65)}      # ... the bands of vs_plan_shape's threshold table (48 and 58)


@pytest.mark.parametrize("arith", [vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA])
def test_n22_over_shallow_rings_under_every_threshold(arith):
    c = cases.ncase("n22")
    tmax = max(cases.expand(l).tbound for l in c.lanes)
    with vs.Engine(0, arith=arith) as eng:
        for depth in RING_DEPTHS:
            ask = 24 if depth == 0.0 else 24 * int(round((24 + depth * tmax) / 24.0))
            for ready in (0, 1, 64):
                tuning = dict(ring_slots=ask)
                if ready:
                    tuning["ready_min"] = ready
                eng.set_tuning(**tuning)
                for ns in (NS, NS - 1):
                    for kind, want in ((vs.VS_KIND_SYNTH, c.want(FAMILY[arith], BATCH, ns)), (vs.VS_KIND_SOURCE, c.flow[:, :ns])):
                        _, name, info = _launch(eng, c.lanes, ns, kind, want, (depth, ready), _names(arith, c.lanes)[kind])
                        slots = info["ring_slots"]
                        rho = (slots - 24) / float(tmax)
                        if depth == 0.0:
                            assert slots < 1.1 * tmax + 56 and slots >= 24 + tmax + 8, (slots, tmax)
                        else:
                            assert slots == ask and DEPTH_BANDS[depth][0] <= rho < DEPTH_BANDS[depth][1], (slots, ask, rho)
            print("VS_ARITH_%s, n22, ring_slots %d asked, %d given (longest tbound %d: %.3f cycles behind a super-step; 1.1 tmax + "
                  "56 = %.1f): SYNTH (%s) and SOURCE at %d and %d samples with ready_min unset, 1 and 64 equal %s and the "
                  "oracle's flow; status 0" % (ARITH_NAME[arith], ask, slots, tmax, rho, 1.1 * tmax + 56,
                                               _names(arith, c.lanes)[vs.VS_KIND_SYNTH].replace(REMARK, ""), NS, NS - 1,
                                               FAMILY_TEXT[FAMILY[arith]]))


# d ---- one long lane among short ones

@functools.lru_cache(maxsize=None)
def _short_long_want():
    """(flow, exact PCM, FMA form behind round2int) of the 48 lanes"""
    lanes = cases.short_long_lanes()
    flow = po.source(lanes, NS)
    A, gain, pre, _ = hostile.lane_sets(lanes, 22)
    return flow, po.synth(lanes, NS), ar.rounded(ar.fma_unrounded(flow, A, gain, pre), "round2int")


@pytest.mark.parametrize("arith", [vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA])
def test_long_period_lanes_among_short_ones(arith):
    """one long-period lane in every 16 of the caller's order; the plan's order (by period) gathers them in its last
    wavefront, whose ring depth the others share: theirs holds ten of their cycles and more"""
    lanes = cases.short_long_lanes()
    n = len(lanes)
    flow, exact, fma = _short_long_want()
    want = exact if arith == vs.VS_ARITH_EXACT else fma
    with vs.Engine(0, arith=arith) as eng:
        for k in (n, 6, 22):                     # the prefixes end behind a long lane
            names = _names(arith, lanes[:k])
            _, name, info = _launch(eng, lanes[:k], NS, vs.VS_KIND_SYNTH, want[:k], "short and long", names[vs.VS_KIND_SYNTH])
            _launch(eng, lanes[:k], NS, vs.VS_KIND_SOURCE, flow[:k], "short and long", names[vs.VS_KIND_SOURCE])
            _launch(eng, lanes[:k], NS, vs.VS_KIND_FILTER, want[:k], "short and long", names[vs.VS_KIND_FILTER], flow=flow[:k])
        same_rows(eng.synth(lanes, NS), want, "vs_synth")
    print("VS_ARITH_%s, %d lanes (long periods at l %% 16 == 5, the rest at 16000 and 22050 Hz, F0 100..250) and the prefixes "
          "6 and 22 x %d samples: %s in %d workgroups, ring %d; SYNTH, FILTER and vs_synth equal %s, SOURCE the oracle's flow" % (
              ARITH_NAME[arith], n, NS, name, info["workgroups"], info["ring_slots"], FAMILY_TEXT[FAMILY[arith]]))


# e ---- layouts

# (samples, pitch): 16-byte stores into padded rows; rows that start 4-byte but not 16-byte aligned; odd pitches (rows only
# 2-byte aligned: sample by sample); the same at an odd length
LAYOUTS = [(ns, ns + d) for ns in (NS, NS - 1) for d in (8, 2, 1, 3)]
# the filter-only kind: (in_pitch, out_pitch, in_off, out_off) at NS samples
FILTER_LAYOUTS = [(NS + 2, NS + 8, 0, 0), (NS + 1, NS, 0, 0), (NS + 8, NS + 1, 0, 0), (NS + 8, NS + 2, 1, 0),
                  (NS + 2, NS + 8, 0, 1), (NS + 2, NS + 2, 1, 1)]


@pytest.mark.parametrize("arith", [vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA])
def test_store_paths_pitches_and_bases(arith):
    c = cases.ncase("n22")
    family = FAMILY[arith]
    names = _names(arith, c.lanes)
    with vs.Engine(0, arith=arith) as eng:
        for ns, pitch in LAYOUTS:
            _launch(eng, c.lanes, ns, vs.VS_KIND_SYNTH, c.want(family, BATCH, ns), "layout", names[vs.VS_KIND_SYNTH], out_pitch=pitch)
            _launch(eng, c.lanes, ns, vs.VS_KIND_SOURCE, c.flow[:, :ns], "layout", names[vs.VS_KIND_SOURCE], out_pitch=pitch)
        for ns in (NS, NS - 1):                  # an output base 2 bytes off
            _launch(eng, c.lanes, ns, vs.VS_KIND_SYNTH, c.want(family, BATCH, ns), "base", names[vs.VS_KIND_SYNTH],
                    out_pitch=ns + 2, out_off=1)
            _launch(eng, c.lanes, ns, vs.VS_KIND_SOURCE, c.flow[:, :ns], "base", names[vs.VS_KIND_SOURCE], out_pitch=ns + 8, out_off=1)
        for in_pitch, out_pitch, in_off, out_off in FILTER_LAYOUTS:
            _launch(eng, c.lanes, NS, vs.VS_KIND_FILTER, c.want(family), "filter layout", names[vs.VS_KIND_FILTER],
                    out_pitch=out_pitch, flow=c.flow, in_pitch=in_pitch, out_off=out_off, in_off=in_off)
    print("VS_ARITH_%s n22: SYNTH (%s) and SOURCE at %d layouts (samples, pitch) %s and with the base 2 bytes off; FILTER (%s) at "
          "%d layouts (in_pitch, out_pitch, samples added to the input base, to the output base) %s: equal %s and the oracle's "
          "flow; padding and guards untouched, the flow's padding holds 0x%X" % (
              ARITH_NAME[arith], names[vs.VS_KIND_SYNTH].replace(REMARK, ""), len(LAYOUTS), LAYOUTS,
              names[vs.VS_KIND_FILTER].replace(REMARK, ""), len(FILTER_LAYOUTS), FILTER_LAYOUTS, FAMILY_TEXT[family], INPUT_PAD))


# f ---- vowel -n behind the narrow kernel

def test_output_noise_passes_behind_the_narrow_kernel(engine):
    c = cases.ncase("n22")
    n = 5000                                     # frames of 50 ms: two whole ones and a tail at 48 kHz, one and a tail at 64 kHz
    lanes = (vs.Lane * BATCH)()
    C.memmove(lanes, c.lanes, C.sizeof(lanes))
    for l in lanes[::2]:
        l.out_snr = 100.0                        # vowel -n 20
    frames = {cases.expand(l).Lframe for l in lanes}
    assert len(frames) == 4 and 2 * min(frames) < n < 2 * max(frames) and n % min(frames) and n % max(frames), frames
    want = po.synth(lanes, n)
    plain = po.synth(c.lanes, n)
    assert (want[::2] != plain[::2]).any(axis=1).all() and np.array_equal(want[1::2], plain[1::2])     # the noise is in the samples
    got, name, info = guarded_plan_launch(engine, lanes, n)
    same_rows(got, want, name)
    _narrow(name, info, BATCH)
    assert name == "vs_synth_kernel<0, 0, false, false>%s + vs_out_power_kernel + vs_out_noise_kernel" % REMARK, name
    total = 0
    with engine.plan(lanes, n) as plan:
        for pitch in LOG_PITCHES:
            recs, ncyc = _want(lanes, n, pitch)
            out, log, cnt = _canary_launch(engine, plan, BATCH, n, vs.VS_KIND_SYNTH, pitch)
            total += _log_held(out, log, cnt, want, recs, ncyc, pitch, ("n22 + vowel -n", pitch))
    print("n22 with vowel -n 20 on every other lane, %d samples: %s equals the oracle without a log and with one (pitches %s: %d "
          "records and the counts too)" % (n, name, list(LOG_PITCHES), total))


# g ---- the wide filter kernel behind the narrow source kernel

def _run_n40(arith):
    family = FAMILY[arith]
    c = cases.ncase("n40")
    shapes = [(BATCH, ns) for ns in hostile.SAMPLE_COUNTS[40] + (NS,)] + [(k, ns) for k in PREFIXES for ns in (49, NS)]
    with vs.Engine(0, arith=arith) as eng:
        total = 0
        for k, ns in shapes:
            lanes, flow, want = c.lanes[:k], c.flow[:k, :ns], c.want(family, k, ns)
            got, name, info = guarded_plan_launch(eng, lanes, ns)
            same_rows(got, want, (name, k, ns))
            # a wide plan's name drops the remark: its shape and its source-only kind say that it is narrow
            assert name == "vs_synth_kernel<0, 1, false, false> + vs_filter_wide_kernel<%d>" % _one(arith), name
            assert info["workgroups"] == -(-k // GROUP), (info, k)
            got_f, fname, info = guarded_plan_launch(eng, lanes, ns, vs.VS_KIND_FILTER, flow=flow)
            same_rows(got_f, want, (fname, k, ns))
            assert fname == "vs_filter_wide_kernel<%d>" % _one(arith) and info["workgroups"] == -(-k // GROUP), (fname, info)
            _launch(eng, lanes, ns, vs.VS_KIND_SOURCE, flow, "n40", _names(arith, lanes)[vs.VS_KIND_SOURCE])
            total += k * ns
            if (k, ns) == (BATCH, NS):
                whole = got
        same_rows(eng.synth(c.lanes, NS), c.want(family), "vs_synth")
    print("VS_ARITH_%s, n40: %s and %s in ceil(n / 16) workgroups on %d shapes %s, %d samples: SYNTH, FILTER and vs_synth equal "
          "%s, SOURCE (%s) the oracle's flow" % (
              ARITH_NAME[arith], name, fname, len(shapes), shapes, total,
              "the oracle" if family == "exact" else "the 40-tap FMA form behind round2int",
              _names(arith, c.lanes)[vs.VS_KIND_SOURCE]))
    return whole


def test_n40_wide_sets_on_long_periods_in_exact_arithmetic():
    _run_n40(vs.VS_ARITH_EXACT)


def test_n40_wide_sets_on_long_periods_in_both_opt_in_contexts():
    fma, f32 = _run_n40(vs.VS_ARITH_FMA), _run_n40(vs.VS_ARITH_F32)
    assert np.array_equal(fma, f32)
    d = fma != cases.ncase("n40").exact
    assert d.sum() > 1000                        # (the split rows: the device ran the FMA form, not the exact one)
    print("n40: the VS_ARITH_FMA and VS_ARITH_F32 contexts give the same bytes, %d samples off the exact oracle's" % d.sum())


# h ---- the host calls

@pytest.mark.parametrize("arith", ARITHS)
def test_vs_synth_and_vs_source_of_n22(arith):
    with vs.Engine(0, arith=arith) as eng:
        for case in ("n22", "n22p1"):
            c = cases.ncase(case)
            with eng.plan(c.lanes, NS) as plan:
                name = plan.kernel_name(vs.VS_KIND_SYNTH)
                _narrow(name, plan.info(), BATCH, _names(arith, c.lanes)[vs.VS_KIND_SYNTH])
            same_rows(eng.synth(c.lanes, NS), c.want(FAMILY[arith]), ("vs_synth", case))
            same_rows(eng.source(c.lanes, NS), c.flow, ("vs_source", case))
            recs, ncyc = cases.log_of(case, LOG_PITCHES[1])
            flow, got_recs, got_ncyc = eng.source(c.lanes, NS, log_cycles=LOG_PITCHES[1])
            same_rows(flow, c.flow, ("vs_source with a log", case))
            assert np.array_equal(got_ncyc, ncyc) and np.array_equal(cases.logref.as_bytes(got_recs), cases.logref.as_bytes(recs))
            print("VS_ARITH_%s, %s: vs_synth (%s) equals %s; vs_source the oracle's flow, log (pitch %d) and counts" % (
                ARITH_NAME[arith], case, name, FAMILY_TEXT[FAMILY[arith]], LOG_PITCHES[1]))


def test_one_long_period_lane_in_the_second_chunk_of_the_host_pipeline(engine):
    """vs_synth cuts the batch into chunks of 16384 utterances with a plan each: only the chunk that holds the long-period
    lane runs on the narrow build"""
    specs, fs, dur, _ = configs.config_specs(3, 16384 + 40)
    lanes, d = vs.lanes_from_specs(specs)
    long_lane = cases.ncase("n22").lanes[0]
    assert cases.expand(long_lane).tbound > cases.WIDE_RING_TBOUND
    C.memmove(C.byref(lanes, (16384 + 7) * C.sizeof(vs.Lane)), C.byref(long_lane), C.sizeof(vs.Lane))
    n = 3000
    with engine.plan(lanes[16384:], n) as plan:
        name, info = plan.kernel_name(vs.VS_KIND_SYNTH), plan.info()
        _narrow(name, info, 40)
    with engine.plan(lanes[:16384], n) as plan:
        assert REMARK not in plan.kernel_name(vs.VS_KIND_SYNTH)
    got = engine.synth(lanes, n)
    pick = [0, 16383, 16384, 16384 + 6, 16384 + 7, 16384 + 8, 16384 + 39]
    assert np.array_equal(got[pick], po.synth([lanes[i] for i in pick], n))
    assert np.array_equal(got[16384:], po.synth([lanes[i] for i in range(16384, 16384 + 40)], n))
    print("vs_synth of 16384 + 40 lanes of config 3 x %d samples with N22's lane 0 at row 16384 + 7: the second chunk's plan "
          "is %s in %d workgroups, ring %d; rows %s and the whole second chunk equal the oracle" % (
              n, name, info["workgroups"], info["ring_slots"], pick))


def test_a_chunk_of_4200_long_period_lanes_over_rings_of_barely_a_cycle(engine):
    c = cases.ncase("n22")
    nl, n = 4200, 3000
    lanes = (vs.Lane * nl)()
    for i in range(nl):
        C.memmove(C.byref(lanes[i]), C.byref(c.lanes[(7 * i) % BATCH]), C.sizeof(vs.Lane))
        lanes[i].seed = 42000 + i
    with engine.plan(lanes, n) as plan:
        name, info = plan.kernel_name(vs.VS_KIND_SYNTH), plan.info()
    _narrow(name, info, nl)
    # the thresholds of vs_plan_shape's table, per wavefront of the plan's order, from how many of the wavefront's
    # longest cycles the ring holds behind a super-step: 64 from 1.65 on, 58, 48 and 32 below
    rho = np.array([(info["ring_slots"] - 24) / float(tb) for _, _, tb in cases.group_rows(lanes)])
    # (the ring is one depth for the whole plan, 1.44 of the batch's longest cycle: the wavefronts of the longer periods
    # run under 58 and 48, those of the shorter ones hold 1.65 cycles and more and wait for all of their lanes)
    assert len(rho) == info["workgroups"] and (rho < 1.65).sum() >= len(rho) // 4 and (rho < 1.45).any(), (rho.min(), rho.max())
    got = engine.synth(lanes, n)
    same_rows(got, po.synth(lanes, n), "vs_synth of a narrow chunk")
    print("vs_synth of %d lanes drawn from N22 x %d samples: %s in %d workgroups, ring %d: %.2f..%.2f of a wavefront's longest "
          "cycle (thresholds below 64 in %d wavefronts: %d under 1.45, %d under 1.33); equals the oracle" % (
              nl, n, name, info["workgroups"], info["ring_slots"], rho.min(), rho.max(), (rho < 1.65).sum(), (rho < 1.45).sum(),
              (rho < 1.33).sum()))


# i ---- the refusal

def test_a_batch_is_refused_whose_lanes_pass_alone(engine):
    lanes = cases.refused_lanes()
    nl, n = len(lanes), 6000
    with pytest.raises(vs.VsError) as e:
        engine.plan(lanes, n)
    assert e.value.code == vs._ffi.VS_ERR_UNSUPPORTED
    # ... and vs_synth of it launches nothing: the caller's rows come back as they were
    out = np.full((nl, n), SENTINEL, dtype=np.int16)
    rc = engine._lib.vs_synth(engine._ctx, lanes, nl, n, out.ctypes.data)
    assert rc == vs._ffi.VS_ERR_UNSUPPORTED and (out == SENTINEL).all()
    narrow = 0
    for i, lane in enumerate(lanes):
        got, name, info = guarded_plan_launch(engine, [lane], n)
        same_rows(got, po.synth([lane], n), (i, name))
        if cases.expand(lane).tbound > cases.WIDE_RING_TBOUND:
            _narrow(name, info, 1)
            narrow += 1
    print("the %d lanes of tests/test_narrow_ref.REFUSED x %d samples: the plan answers VS_ERR_UNSUPPORTED and vs_synth writes "
          "nothing; each lane alone equals the oracle (%d of them on the narrow build, the 44.1 kHz ones on the 64-column ring)" % (
              nl, n, narrow))
