"""The two opt-in arithmetics of the fused synthesis kernels, byte for byte against their numpy restatements
(tests/arith_ref.py; the operation orders are written out in include/voice_synth.h):

  a. VS_ARITH_FMA on the one-wave kernel and the filter-only kind: the FMA form behind round2int (VS_ARITH_F32 runs the
     same there);
  b. VS_ARITH_FMA on the wave-specialised kernels: the FMA form behind nearest-even and the saturating conversion;
  c. VS_ARITH_F32 on the wave-specialised kernels: the packed single-precision form behind half-up;
  d. b and c with two and three roles, 1, 2 and 4 groups per workgroup, the pre-emphasis-1 instantiation and the general
     one, and both filter loops (the wavefront's lanes share a position / each lane has its own);
  e. the store paths: 16-byte stores against sample-by-sample ones, odd pitches, padding and guard samples left alone;
  f. what a wrong kernel would show: the FMA form differs from the exact oracle on the split-sum lanes, the two FMA
     families differ from each other on the tie lanes.

The cases and the conditions under which they mean something are built and asserted on the CPU in
tests/test_arith_ref.py; here the device runs them.  Batches have 130 lanes (two whole groups of 64 utterances and a
ragged one) and prefixes of 1, 63 and 65 lanes; sample counts 1, 23 .. 49 and 999 (odd: every store goes sample by
sample) and 1000 (16-byte stores and a tail of 16).  Every test prints what it compared (pytest -s):
profiles/arith_restatements.txt keeps those lines."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_arith_ref as cases  # noqa: E402
from test_arith_ref import BATCH, NS, PREFIXES, SAMPLE_COUNTS  # noqa: E402
from gpu_support import guarded_plan_launch, same_rows, ws_engine  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024
SYNC_BYTES = 10 * 64 * 4 + 16      # a group's progress words in the three-role kernel, and the rounding of its region
PREFIX_COUNTS = (25, NS)     # the sample counts the shorter batches run at
ARITH_NAME = {vs.VS_ARITH_FMA: "fma", vs.VS_ARITH_F32: "f32"}


def _want(c, family, lanes, ns):
    if family == "f32":
        return c.f32[:lanes, :ns]
    return c.fma(family, lanes, ns)


def _shapes():
    """(lanes, samples) of every launch of a grid point: the whole batch at every sample count, the prefixes at two"""
    return [(BATCH, ns) for ns in SAMPLE_COUNTS] + [(k, ns) for k in PREFIXES[:-1] for ns in PREFIX_COUNTS]


# a ---- the half-down family: the one-wave kernel and the filter-only kind

@pytest.mark.parametrize("arith", [vs.VS_ARITH_FMA, vs.VS_ARITH_F32])
def test_one_wave_and_filter_only_kernels_run_the_fma_form_behind_round2int(arith):
    with vs.Engine(0, arith=arith) as eng:
        eng.set_tuning(kernel=vs.VS_KERNEL_SINGLE)
        for pre1 in (False, True):
            c = cases.batch(pre1)
            for k, ns in _shapes():
                want = _want(c, "round2int", k, ns)
                lanes = c.lanes[:k]
                got, name, _ = guarded_plan_launch(eng, lanes, ns)
                assert name == "vs_synth_kernel<1, 0, false, false>", name
                same_rows(got, want, (name, k, ns))
                got, fname, _ = guarded_plan_launch(eng, lanes, ns, vs.VS_KIND_FILTER, flow=c.flow[:k, :ns])
                assert fname == "vs_synth_kernel<1, 2, false, false>", fname
                same_rows(got, want, (fname, k, ns))
                same_rows(eng.filter(lanes, c.flow[:k, :ns]), want, ("vs_filter", k, ns))
            print("VS_ARITH_%s, %s: %s and %s (launch and vs_filter) equal the FMA form behind round2int on %d shapes" % (
                ARITH_NAME[arith].upper(), "pre-emphasis 1" if pre1 else "mixed pre-emphasis", name, fname, len(_shapes())))


# b, c, d ---- the wave-specialised kernels

WS_GRID = [(roles, pairs, ready) for roles in (2, 3) for pairs in (1, 2, 4) for ready in ((64, 32) if roles == 2 else (0,))]
LOOP = {64: "shared position", 32: "own positions", 0: "shared position"}


@pytest.mark.parametrize("roles,pairs,ready", WS_GRID)
@pytest.mark.parametrize("arith", [vs.VS_ARITH_FMA, vs.VS_ARITH_F32])
def test_wave_specialised_kernels_equal_their_restatement(arith, roles, pairs, ready):
    family = "nearest_even" if arith == vs.VS_ARITH_FMA else "f32"
    with ws_engine(arith, roles, pairs, ready) as eng:
        for pre1 in (False, True):
            c = cases.batch(pre1)
            for k, ns in _shapes():
                got, name, info = guarded_plan_launch(eng, c.lanes[:k], ns)
                inst = all(l.pre_emphasis == 1.0 for l in c.lanes[:k])    # (the first lanes of the mixed batch may all have 1)
                assert inst == pre1 or k < BATCH
                assert name == "vs_synth_ws_kernel<%d, %s, %d>" % (arith, "true" if inst else "false", roles), name
                assert pairs * (info["lds_bytes"] + SYNC_BYTES) <= LDS_LIMIT, info     # the plan kept the groups asked for
                same_rows(got, _want(c, family, k, ns), (name, pairs, ready, k, ns))
            print("%s, %d group(s) per workgroup, %s, ring %d: equals %s on %d shapes" % (
                name, pairs, LOOP[ready], info["ring_slots"],
                "the single-precision form behind half-up" if family == "f32" else "the FMA form behind nearest-even",
                len(_shapes())))


def test_the_plans_own_choice_of_kernel_equals_the_restatements():
    """no tuning: what a caller gets for this batch (a half-filled chip: three roles, the library's rings), through
    vs_synth as well as through a launch"""
    for arith, family in ((vs.VS_ARITH_FMA, "nearest_even"), (vs.VS_ARITH_F32, "f32")):
        with vs.Engine(0, arith=arith) as eng:
            for pre1 in (False, True):
                c = cases.batch(pre1)
                for ns in (999, NS):
                    got, name, info = guarded_plan_launch(eng, c.lanes, ns)
                    assert name.startswith("vs_synth_ws_kernel<%d, %s," % (arith, "true" if pre1 else "false")), name
                    same_rows(got, _want(c, family, BATCH, ns), (name, ns))
                    same_rows(eng.synth(c.lanes, ns), _want(c, family, BATCH, ns), ("vs_synth", name, ns))
                print("untuned %s, ring %d: launch and vs_synth equal the restatement at 999 and 1000 samples" % (
                    name, info["ring_slots"]))


# e ---- store paths

# (samples, pitch): 16-byte stores into padded rows; an odd pitch (rows only 2-byte aligned: sample by sample); an odd
# length in even rows (16-byte stores and a tail of 15); an odd length in rows of that pitch
LAYOUTS = [(NS, NS + 8), (NS, NS + 1), (NS - 1, NS), (NS - 1, NS - 1), (NS, NS + 3)]


def test_store_paths_and_pitches():
    runs = [("one-wave", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_SINGLE), "round2int"),
            ("two roles", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=64), "nearest_even"),
            ("two roles, own positions", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=32), "nearest_even"),
            ("three roles", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=3), "nearest_even"),
            ("two roles", vs.VS_ARITH_F32, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=64), "f32"),
            ("two roles, own positions", vs.VS_ARITH_F32, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2, ready_min=32), "f32"),
            ("three roles", vs.VS_ARITH_F32, dict(kernel=vs.VS_KERNEL_WS, ws_roles=3), "f32")]
    c = cases.batch(False)
    for label, arith, tuning, family in runs:
        with vs.Engine(0, arith=arith) as eng:
            eng.set_tuning(**tuning)
            outs = {}
            for ns, pitch in LAYOUTS:
                got, name, _ = guarded_plan_launch(eng, c.lanes, ns, out_pitch=pitch)
                same_rows(got, _want(c, family, BATCH, ns), (name, ns, pitch))
                outs[(ns, pitch)] = got
                if label == "one-wave":          # the filter-only kind reads as it writes: the flow at that pitch too
                    got, fname, _ = guarded_plan_launch(eng, c.lanes, ns, vs.VS_KIND_FILTER, out_pitch=pitch, flow=c.flow[:, :ns],
                                            in_pitch=pitch)
                    same_rows(got, _want(c, family, BATCH, ns), (fname, ns, pitch))
            # (implied by the comparisons above) 16-byte stores and sample-by-sample stores give the same bytes
            assert np.array_equal(outs[(NS, NS + 8)], outs[(NS, NS + 1)])
            assert np.array_equal(outs[(NS - 1, NS)], outs[(NS, NS + 1)][:, :NS - 1])
            print("VS_ARITH_%s %s (%s): %d layouts (samples, pitch) %s equal the restatement; padding and guards untouched" % (
                ARITH_NAME[arith].upper(), label, name, len(LAYOUTS), LAYOUTS))


# f ---- what a wrong kernel would show

def test_a_kernel_in_another_form_or_rounding_would_fail():
    """the device's FMA output differs from the exact oracle on the split-sum rows (a kernel that ran the exact form
    would not), the two FMA families differ from each other on the tie rows (a kernel with the other family's rounding
    would not), and single precision differs from both.  All of it follows from the comparisons above."""
    c = cases.batch(False)
    cases.check_batch_conditions(c, False)
    exact = pyoracle.synth(c.lanes, NS)
    assert np.array_equal(exact, pyoracle.filter(c.lanes, c.flow))
    got = {}
    for key, arith, tuning in (("one-wave", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_SINGLE)),
                               ("ws", vs.VS_ARITH_FMA, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2)),
                               ("f32", vs.VS_ARITH_F32, dict(kernel=vs.VS_KERNEL_WS, ws_roles=2))):
        with vs.Engine(0, arith=arith) as eng:
            eng.set_tuning(**tuning)
            got[key] = guarded_plan_launch(eng, c.lanes, NS)[0]
    sp, tie = c.rows("split"), c.rows("tie")
    for key in ("one-wave", "ws"):
        d = got[key][sp] != exact[sp]
        assert d.sum() >= 10 and d.any(axis=1).sum() >= 3, (key, d.sum())
        print("%s kernel under FMA: differs from the exact oracle in %d of %d samples of the split-sum rows (%d rows)" % (
            key, d.sum(), d.size, d.any(axis=1).sum()))
    fam = got["one-wave"][tie] != got["ws"][tie]
    assert fam.mean() >= 0.10, fam.mean()
    assert np.array_equal(got["one-wave"][tie] != got["ws"][tie], c.fma("round2int")[tie] != c.fma("nearest_even")[tie])
    up = got["f32"][tie] != got["ws"][tie]
    assert up.mean() >= 0.10 and (got["f32"][tie] != got["one-wave"][tie]).mean() >= 0.10
    print("tie rows: the one-wave and the wave-specialised kernel differ in %.1f %% of the samples under FMA; single "
          "precision differs from them in %.1f %% and %.1f %%" % (100 * fam.mean(), 100 * (got["f32"][tie] != got["one-wave"][tie]).mean(),
                                                              100 * up.mean()))
