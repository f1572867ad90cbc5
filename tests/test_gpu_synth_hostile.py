"""The synthesis filter kernels on hostile sets, byte for byte against their forms (include/voice_synth.h):

  a. H22, the one-wave kernel (synth kind and filter-only kind) and vs_filter: the oracle in VS_ARITH_EXACT, the FMA form
     behind round2int in VS_ARITH_FMA and VS_ARITH_F32;
  b. H22, the wave-specialised kernels (two roles whose lanes share a position or have their own, three roles; 1 and 4
     groups per workgroup; both pre-emphasis instantiations): the oracle, the FMA form behind nearest-even, the
     single-precision form behind half-up;
  c. H40, the wide kernel: the oracle, and the 40-tap FMA form behind round2int in both opt-in contexts;
  d. layouts: pitches of n + 8, n + 2 (rows 4-byte but not 16-byte aligned), n + 1 and n + 3, an odd length, and for the
     filter-only kind an input pitch of its own and bases 2 bytes off; padding and guards untouched;
  e. what a wrong wide kernel would show.

The batches and the conditions under which they mean something are built and asserted on the CPU in
tests/test_synth_hostile_ref.py: lanes whose rounding argument passes int16, int32 and int64, and lanes whose state
leaves the finite numbers inside the row.  A row is compared up to and including the first sample f whose state is not
finite; behind it only |out| <= 32767 is asserted (what the header promises).  Every test prints what it compared
(pytest -s): profiles/synth_hostile_sets.txt keeps those lines."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_synth_hostile_ref as cases  # noqa: E402
from test_synth_hostile_ref import BATCH, NS, PREFIXES, SAMPLE_COUNTS, compared  # noqa: E402
from gpu_support import INPUT_PAD, guarded_plan_launch, ws_engine  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024
SYNC_BYTES = 10 * 64 * 4 + 16      # a group's progress words in the three-role kernel, and the rounding of its region
ARITHS = (vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA, vs.VS_ARITH_F32)
ARITH_NAME = {vs.VS_ARITH_EXACT: "EXACT", vs.VS_ARITH_FMA: "FMA", vs.VS_ARITH_F32: "F32"}
# the form each kernel family runs in each context (the pairing of tests/test_gpu_arith.py)
ONE_WAVE_FAMILY = {vs.VS_ARITH_EXACT: "exact", vs.VS_ARITH_FMA: "round2int", vs.VS_ARITH_F32: "round2int"}
WS_FAMILY = {vs.VS_ARITH_EXACT: "exact", vs.VS_ARITH_FMA: "nearest_even", vs.VS_ARITH_F32: "f32"}


def _held(got, want_f, what):
    """got against (want, f): equal on n <= f, |out| <= 32767 everywhere; returns the number of samples compared"""
    want, f = want_f
    assert got.shape == want.shape, what
    seen = compared(f, got.shape[1])
    bad = (got != want) & seen
    assert not bad.any(), (what, np.argwhere(bad)[:8], got[bad][:8], want[bad][:8])
    assert (got != -32768).all(), (what, np.argwhere(got == -32768)[:8])
    return int(seen.sum())


def _shapes(P):
    """(lanes, samples) of every launch of a grid point: the whole batch at every sample count, the prefixes at two"""
    few = (25, NS) if P == 22 else (49, NS)
    return [(BATCH, ns) for ns in SAMPLE_COUNTS[P]] + [(k, ns) for k in PREFIXES[:-1] for ns in few]


# a ---- H22: the one-wave kernel, the filter-only kind, vs_filter

@pytest.mark.parametrize("arith", ARITHS)
def test_h22_one_wave_and_filter_only_kernels(arith):
    family = ONE_WAVE_FAMILY[arith]
    one = vs.VS_ARITH_FMA if arith == vs.VS_ARITH_F32 else arith
    with vs.Engine(0, arith=arith) as eng:
        eng.set_tuning(kernel=vs.VS_KERNEL_SINGLE)
        for case in ("h22", "h22p1"):
            c = cases.hcase(case)
            total = 0
            for k, ns in _shapes(22):
                want = c.want(family, k, ns)
                lanes = c.lanes[:k]
                got, name, _ = guarded_plan_launch(eng, lanes, ns)
                assert name.startswith("vs_synth_kernel<%d, 0, false, " % one), name
                total += _held(got, want, (name, k, ns))
                got, fname, _ = guarded_plan_launch(eng, lanes, ns, vs.VS_KIND_FILTER, flow=c.flow[:k, :ns])
                assert fname.startswith("vs_synth_kernel<%d, 2, false, " % one), fname
                _held(got, want, (fname, k, ns))
                _held(eng.filter(lanes, c.flow[:k, :ns]), want, ("vs_filter", k, ns))
            print("VS_ARITH_%s, %s: %s and %s (launch and vs_filter) equal %s on %d shapes, %d samples each" % (
                ARITH_NAME[arith], case, name, fname, "the oracle" if family == "exact" else "the FMA form behind round2int",
                len(_shapes(22)), total))


# b ---- H22: the wave-specialised kernels

WS_GRID = [(2, 1, 64), (2, 1, 32), (2, 4, 64), (2, 4, 32), (3, 1, 0), (3, 4, 0)]      # (roles, groups per workgroup, ready_min)
LOOP = {64: "shared position", 32: "own positions", 0: "shared position"}
FAMILY_TEXT = {"exact": "the oracle", "nearest_even": "the FMA form behind nearest-even", "f32": "the single-precision form behind half-up",
               "round2int": "the FMA form behind round2int"}


@pytest.mark.parametrize("roles,pairs,ready", WS_GRID)
@pytest.mark.parametrize("arith", ARITHS)
def test_h22_wave_specialised_kernels(arith, roles, pairs, ready):
    family = WS_FAMILY[arith]
    with ws_engine(arith, roles, pairs, ready) as eng:
        for case in ("h22", "h22p1"):
            c = cases.hcase(case)
            total = 0
            for k, ns in _shapes(22):
                got, name, info = guarded_plan_launch(eng, c.lanes[:k], ns)
                inst = all(l.pre_emphasis == 1.0 for l in c.lanes[:k])
                assert inst == (case == "h22p1") or k < BATCH
                assert name == "vs_synth_ws_kernel<%d, %s, %d>" % (arith, "true" if inst else "false", roles), name
                assert pairs * (info["lds_bytes"] + SYNC_BYTES) <= LDS_LIMIT, info     # the plan kept the groups asked for
                total += _held(got, c.want(family, k, ns), (name, pairs, ready, k, ns))
            print("%s, %s, %d group(s) per workgroup, %s, ring %d: equals %s on %d shapes, %d samples" % (
                case, name, pairs, LOOP[ready], info["ring_slots"], FAMILY_TEXT[family], len(_shapes(22)), total))


@pytest.mark.parametrize("arith", ARITHS)
def test_h22_through_vs_synth_and_vs_filter(arith):
    """no tuning: the kernel the plan picks for this batch, through the host calls"""
    with vs.Engine(0, arith=arith) as eng:
        for case in ("h22", "h22p1"):
            c = cases.hcase(case)
            with eng.plan(c.lanes, NS) as plan:
                name = plan.kernel_name(vs.VS_KIND_SYNTH)
            family = WS_FAMILY[arith] if name.startswith("vs_synth_ws_kernel") else ONE_WAVE_FAMILY[arith]
            a = _held(eng.synth(c.lanes, NS), c.want(family), ("vs_synth", name))
            b = _held(eng.filter(c.lanes, c.flow), c.want(ONE_WAVE_FAMILY[arith]), ("vs_filter", case))
            print("VS_ARITH_%s, %s: vs_synth (%s) equals %s, vs_filter %s; %d and %d samples" % (
                ARITH_NAME[arith], case, name, FAMILY_TEXT[family], FAMILY_TEXT[ONE_WAVE_FAMILY[arith]], a, b))


# c ---- H40: the wide kernel

def _run_h40(arith):
    """every shape of H40 in a context of that arithmetic, both kinds and both host calls; the rows of the whole batch
    at NS samples"""
    family = ONE_WAVE_FAMILY[arith]
    one = vs.VS_ARITH_FMA if arith == vs.VS_ARITH_F32 else arith
    c = cases.hcase("h40")
    with vs.Engine(0, arith=arith) as eng:
        total = 0
        for k, ns in _shapes(40):
            want = c.want(family, k, ns)
            got, name, _ = guarded_plan_launch(eng, c.lanes[:k], ns)
            wide = True                          # (lane 0 has 40 taps: every prefix is wide)
            assert name.endswith("vs_filter_wide_kernel<%d>" % one) == wide, (name, k)
            total += _held(got, want, (name, k, ns))
            got_f, fname, _ = guarded_plan_launch(eng, c.lanes[:k], ns, vs.VS_KIND_FILTER, flow=c.flow[:k, :ns])
            assert (fname == "vs_filter_wide_kernel<%d>" % one) == wide, (fname, k)
            _held(got_f, want, (fname, k, ns))
            if (k, ns) == (BATCH, NS):
                whole, whole_name, whole_fname = got, name, fname
        assert c.order[0] > 22
        _held(eng.synth(c.lanes, NS), c.want(family), ("vs_synth", whole_name))
        _held(eng.filter(c.lanes, c.flow), c.want(family), ("vs_filter", whole_fname))
        print("VS_ARITH_%s, h40: %s and %s (launches, vs_synth and vs_filter) equal %s on %d shapes, %d samples" % (
            ARITH_NAME[arith], whole_name, whole_fname,
            "the oracle" if family == "exact" else "the 40-tap FMA form behind round2int", len(_shapes(40)), total))
    return whole


def test_h40_wide_kernel_in_exact_arithmetic():
    _run_h40(vs.VS_ARITH_EXACT)


def test_h40_wide_kernel_runs_the_40_tap_fma_form_in_both_opt_in_contexts():
    fma, f32 = _run_h40(vs.VS_ARITH_FMA), _run_h40(vs.VS_ARITH_F32)
    assert np.array_equal(fma, f32)
    print("h40: the VS_ARITH_FMA and VS_ARITH_F32 contexts give the same bytes")


# d ---- layouts

# (samples, pitch): 16-byte stores into padded rows; rows that start 4-byte but not 16-byte aligned; an odd pitch (rows
# only 2-byte aligned: sample by sample); an odd length in even rows; another odd pitch
LAYOUTS = [(NS, NS + 8), (NS, NS + 2), (NS, NS + 1), (NS - 1, NS), (NS, NS + 3)]
# the filter-only kind: (in_pitch, out_pitch, in_off, out_off) at NS samples
FILTER_LAYOUTS = [(NS + 2, NS + 8, 0, 0), (NS + 1, NS, 0, 0), (NS + 8, NS + 1, 0, 0), (NS + 8, NS + 2, 1, 0),
                  (NS + 2, NS + 8, 0, 1), (NS + 2, NS + 2, 1, 1)]
LAYOUT_RUNS = [("h40", "wide", vs.VS_ARITH_EXACT, {}, "exact", True),
               ("h40", "wide", vs.VS_ARITH_FMA, {}, "round2int", True),
               ("h22", "one-wave", vs.VS_ARITH_EXACT, dict(kernel=vs.VS_KERNEL_SINGLE), "exact", True),
               ("h22", "one-wave", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_SINGLE), "round2int", True),
               ("h22", "two roles", vs.VS_ARITH_EXACT, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=64), "exact", False),
               ("h22", "two roles, own positions", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=32),
                "nearest_even", False),
               ("h22", "three roles", vs.VS_ARITH_EXACT, dict(kernel=vs.VS_KERNEL_WS, ws_roles=3), "exact", False),
               ("h22", "three roles", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=3), "nearest_even", False)]


@pytest.mark.parametrize("case,label,arith,tuning,family,filter_kind", LAYOUT_RUNS,
                         ids=["%s-%s-%s" % (r[0], r[1].replace(" ", "_").replace(",", ""), ARITH_NAME[r[2]]) for r in LAYOUT_RUNS])
def test_store_paths_pitches_and_bases(case, label, arith, tuning, family, filter_kind):
    c = cases.hcase(case)
    with vs.Engine(0, arith=arith) as eng:
        if tuning:
            eng.set_tuning(**tuning)
        outs = {}
        for ns, pitch in LAYOUTS:
            got, name, _ = guarded_plan_launch(eng, c.lanes, ns, out_pitch=pitch)
            _held(got, c.want(family, BATCH, ns), (name, ns, pitch))
            outs[(ns, pitch)] = got
        # the 16-byte and the sample-by-sample paths give the same bytes (on the samples anything is promised for)
        seen = compared(c.want(family)[1], NS)
        for key in LAYOUTS[1:]:
            assert np.array_equal(outs[key][seen[:, :key[0]]], outs[LAYOUTS[0]][:, :key[0]][seen[:, :key[0]]]), key
        print("VS_ARITH_%s %s, %s (%s): %d layouts (samples, pitch) %s equal %s; padding and guards untouched" % (
            ARITH_NAME[arith], case, label, name, len(LAYOUTS), LAYOUTS, FAMILY_TEXT[family]))
        if filter_kind:
            for in_pitch, out_pitch, in_off, out_off in FILTER_LAYOUTS:
                got, fname, _ = guarded_plan_launch(eng, c.lanes, NS, vs.VS_KIND_FILTER, out_pitch=out_pitch, flow=c.flow,
                                                     in_pitch=in_pitch, out_off=out_off, in_off=in_off)
                _held(got, c.want(family), (fname, in_pitch, out_pitch, in_off, out_off))
                assert np.array_equal(got[seen], outs[LAYOUTS[0]][seen]), (fname, in_pitch, out_pitch, in_off, out_off)
            print("VS_ARITH_%s %s, filter-only kind (%s): %d layouts (in_pitch, out_pitch, samples added to the input base, "
                  "to the output base) %s equal %s; the flow's padding holds 0x%X" % (
                      ARITH_NAME[arith], case, fname, len(FILTER_LAYOUTS), FILTER_LAYOUTS, FAMILY_TEXT[family], INPUT_PAD))


# e ---- what a wrong kernel would show

def test_a_wide_kernel_in_another_form_would_fail():
    """the device's FMA output differs from the exact oracle on the split-sum rows whose taps sit above tap 22 (a wide
    kernel that ran the exact form, or the FMA form over fewer taps or with the partial sums swapped, would not give
    these bytes), and its exact output does not"""
    c = cases.hcase("h40")
    cases.check_conditions(c)
    sp = c.rows("split")
    got = {}
    for arith in (vs.VS_ARITH_EXACT, vs.VS_ARITH_FMA):
        with vs.Engine(0, arith=arith) as eng:
            got[arith], name, _ = guarded_plan_launch(eng, c.lanes, NS)
            assert name.endswith("vs_filter_wide_kernel<%d>" % arith), name
    d = got[vs.VS_ARITH_FMA][sp] != c.exact[sp]
    assert d.sum() >= 10 and d.any(axis=1).sum() >= 3, (d.sum(), d.any(axis=1))
    assert np.array_equal(d, c.want("round2int")[0][sp] != c.exact[sp])
    assert np.array_equal(got[vs.VS_ARITH_EXACT][sp], c.exact[sp])
    print("h40, split-sum rows (taps %s): the wide kernel under FMA differs from the exact oracle in %d of %d samples on %d of "
          "%d rows; in exact arithmetic in none" % (" ".join(str(t) for t in cases.SPLIT_TAPS[40]), d.sum(), d.size,
                                                    d.any(axis=1).sum(), len(sp)))
