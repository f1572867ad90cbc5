"""The output-noise kernels of "vowel -n" (csrc/vs_out_noise.hip: vs_out_power_kernel, vs_out_power_fill_kernel,
vs_out_noise_kernel) on what the rest of the suite never feeds them, byte for byte against the oracle:

  1. frames whose noise width lies in every class of the kernel (zero, small, plain, big), octets of eight samples whose
     two quads lie in frames of different classes, full-scale power sums, both clamps, at three frame lengths;
  2. row lengths around the three tails (last frame, last octet, second quad) and around the segments of 2048 samples;
  3. rows that are only 2-byte aligned (the scalar instantiations), with the padding and the guards left alone;
  4. the same stage behind the wide filter kernel, behind the fused kernels (power taken along and filled in, streamed,
     and with super-steps rounded again) and under the two opt-in arithmetics;
  5. what the library refuses.

The cases and the conditions under which they mean something are built and asserted on the CPU in
tests/test_onoise_ref.py (with the restatement tests/onoise_ref.py); here the device runs them.  Every comparison is
np.array_equal.  Every test prints what it ran (pytest -s): profiles/onoise_hostile_signals.txt keeps those lines."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onoise_ref as on  # noqa: E402
import test_onoise_ref as cases  # noqa: E402
from gpu_support import INPUT_PAD, GuardedRows  # noqa: E402

pytestmark = pytest.mark.gpu


def _kernel_name(engine, lanes, n, kind):
    with engine.plan(lanes, n) as plan:
        return plan.kernel_name(kind)


def _same(got, want, what=""):
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8])


def _line(c):
    noisy, W, aux = cases.restated(c)
    return cases.describe(c, W, aux)


# 1 ---- width classes and mixed octets

@pytest.mark.parametrize("fs", cases.RATES)
def test_width_classes_and_mixed_octets(engine, fs):
    line = cases.check_class_conditions(fs)
    c = cases.class_case(fs)
    name = _kernel_name(engine, c.lanes, c.n, vs.VS_KIND_FILTER)
    assert "vs_out_power_kernel" in name and "_fill_" not in name and "vs_out_noise_kernel" in name, name
    got = engine.filter(c.lanes, c.flow)
    _same(got, c.want, fs)
    off = c.snr == 0
    _same(got[off], c.quiet[off], "lanes without noise")
    print("%s; %s" % (line, name))


# 2 ---- tails and segments

@pytest.mark.parametrize("fs", [22050, 2000])
def test_tails(engine, fs):
    L = on.frame_length(fs)
    for n in cases.tail_sizes(L) + ([2049, 2048] if fs == 22050 else []):
        c = cases.tail_case(fs, n)
        got = engine.filter(c.lanes, c.flow)
        _same(got, c.want, (fs, n))
        print("tails: %s, segments %d" % (_line(c), (n + 2047) // 2048))


# 3 ---- rows that are only 2-byte aligned

def _layout_launch(engine, c, out_pitch, out_off, in_pitch, in_off, what):
    """the case through Plan.launch into sentinel-filled memory (offsets in bytes); returns the rows, with the padding and
    the guards untouched"""
    R, n = len(c.lanes), c.n
    with engine.scope() as dev:
        out = GuardedRows(R, n, out_pitch, out_off).on(dev)
        in_d = dev.room((R * in_pitch + 1) * 2)
        plan = dev.plan(c.lanes, n)
        staged = np.full((R, in_pitch), INPUT_PAD, dtype=np.int16)      # the padding of the input is not silence
        staged[:, :n] = c.flow
        engine.dev_upload(in_d + in_off, staged)
        plan.launch(vs.VS_KIND_FILTER, out.first(out_pitch, out_off), out_pitch=out_pitch, in_ptr=in_d + in_off,
                    in_pitch=in_pitch)
        plan.status()
        name = plan.kernel_name(vs.VS_KIND_FILTER)
        return out.rows_back(out_pitch, out_off, what), name


def test_rows_that_are_only_two_byte_aligned(engine):
    c = cases.class_case(22050)
    n = c.n
    even, odd = n + 3, n + 2
    assert even % 2 == 0 and odd % 2 == 1
    layouts = [("aligned", even, 0, even, 0), ("odd out_pitch", odd, 0, even, 0), ("out_ptr + 2", even, 2, even, 0),
               ("odd in_pitch", even, 0, odd, 0), ("in_ptr + 2", even, 0, even, 2)]
    for what, out_pitch, out_off, in_pitch, in_off in layouts:
        rows, name = _layout_launch(engine, c, out_pitch, out_off, in_pitch, in_off, what)
        _same(rows, c.want, what)
        print("layout %-13s out_pitch %d + %d B, in_pitch %d + %d B: %d lanes x %d samples, padding and guards untouched; %s" % (
            what, out_pitch, out_off, in_pitch, in_off, len(c.lanes), n, name))


@pytest.mark.parametrize("n", [4401, 4404, 4405])
def test_aligned_rows_stop_at_their_length(engine, n):
    assert n % 8 in (1, 4, 5)
    c = cases.Case(22050, n, 94)
    pitch = (n + 9) & ~1
    rows, name = _layout_launch(engine, c, pitch, 0, pitch, 0, n)
    _same(rows, c.want, n)
    print("aligned, n %% 8 = %d: %s, pitch %d, padding and guards untouched" % (n % 8, _line(c), pitch))


# 4 ---- behind the other producers

def test_behind_the_wide_filter_kernel(engine):
    c = cases.class_case(22050, 94, 23)
    name = _kernel_name(engine, c.lanes, c.n, vs.VS_KIND_FILTER)
    assert "vs_filter_wide_kernel" in name, name
    _same(c.want, cases.class_case(22050).want, "an identity set of 23 taps is the identity")
    got = engine.filter(c.lanes, c.flow)
    _same(got, c.want)
    print("wide: %s; %s" % (_line(c), name))


def test_behind_the_fused_kernels():
    lanes, fs, n = cases.synth_case()
    want = pyoracle.synth(lanes, n)
    runs = [("the plan's own choice", {}, True), ("one-wave kernel", dict(kernel=vs.VS_KERNEL_SINGLE), False),
            ("super-steps rounded again", dict(fault=vs.VS_FAULT_REROUND), True)]
    for what, tuning, fill in runs:
        with vs.Engine(0) as eng:
            if tuning:
                eng.set_tuning(**tuning)
            name = _kernel_name(eng, lanes, n, vs.VS_KIND_SYNTH)
            assert ("vs_out_power_fill_kernel" in name) == fill and ("vs_out_power_kernel" in name) == (not fill), name
            assert "vs_out_noise_kernel" in name
            got = eng.synth(lanes, n)
        _same(got, want, what)
        print("synth, %s: %d lanes x %d samples, %d samples differ from the oracle; %s" % (
            what, len(lanes), n, (got != want).sum(), name))


@pytest.mark.parametrize("arith", [vs.VS_ARITH_FMA, vs.VS_ARITH_F32])
@pytest.mark.parametrize("fs", cases.RATES)
def test_identity_lanes_under_the_other_arithmetics(fs, arith):
    """the identity filter is exact in all three arithmetics, so the noisy rows are still the oracle's"""
    c = cases.class_case(fs)
    with vs.Engine(0, arith=arith) as eng:
        name = _kernel_name(eng, c.lanes, c.n, vs.VS_KIND_FILTER)
        got = eng.filter(c.lanes, c.flow)
    _same(got, c.want, (fs, arith))
    print("arith %d: %s; %s" % (arith, _line(c), name))


# 5 ---- refusals

def test_refusals(engine):
    flow = cases.rows_for(2000, 405)[:1]
    lane = cases.identity_lane(1999, 100.0, 9)
    with pytest.raises(vs.VsError) as e:            # frames of no length (vowel_new.c:361-363 gives Lframe 0)
        engine.filter([lane], flow)
    assert e.value.code == _ffi.VS_ERR_UNSUPPORTED
    quiet = np.clip(flow, -32767, 32767)
    lane.out_snr = 0.0                              # ... which only the noise minds
    _same(engine.filter([lane], flow), quiet)
    lane = cases.identity_lane(2000, 100.0, 9)
    want = pyoracle.filter([lane], flow)
    assert (want != quiet).any()
    _same(engine.filter([lane], flow), want)
    # vs_lane_validate has no word on out_snr: only out_snr > 0 asks for noise, so NaN and negative values mean "off",
    # on the device as in the oracle
    for snr in (float("nan"), -1.0, -0.0, float("-inf")):
        lane = cases.identity_lane(2000, snr, 9)
        assert vs.load().vs_lane_validate(vs.C.byref(lane)) == _ffi.VS_OK
        _same(pyoracle.filter([lane], flow), quiet, snr)
        _same(engine.filter([lane], flow), quiet, snr)
        lane.fs = 1999
        _same(engine.filter([lane], flow), quiet, snr)
    print("refusals: out_snr > 0 at fs 1999 VS_ERR_UNSUPPORTED, accepted at fs 2000; NaN and negative out_snr mean off")
