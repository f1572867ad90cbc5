"""Explicit coefficient sets of up to MAX_ORDER = 40 taps (vowel_new.c:33).

The reference's recurrence (vowel_new.c:279-281, 287-289) is written for any Order; only its ten
tables stop at 22.  Sets of 23..40 taps take the un-fused wide path (source kernel -> flow in HBM ->
vs_filter_wide_kernel); lower orders ride the fused kernels with zeros in the missing taps.
Bit-exact against the CPU oracle (which tests/test_oracle_custom.py holds to a literal statement of
the loop) in VS_ARITH_EXACT, within +-1 LSB in VS_ARITH_FMA."""
import ctypes as C

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ORDERS = [1, 2, 5, 21, 22, 23, 24, 30, 31, 39, 40]


def _lanes(n):
    return configs.wide_order_lanes([ORDERS[i % len(ORDERS)] for i in range(n)])


@pytest.mark.parametrize("n_samples", [16000, 4999, 47, 1])
def test_sets_of_every_order_bit_exact(engine, n_samples):
    lanes, fs, dur = _lanes(200)
    got = engine.synth(lanes, n_samples)
    assert np.array_equal(got, po.synth(lanes, n_samples))
    assert np.array_equal(engine.source(lanes, n_samples), po.source(lanes, n_samples))


def test_the_plan_is_wide_and_says_so(engine):
    lanes, fs, dur = _lanes(70)
    with engine.plan(lanes, 1000) as plan:
        assert "vs_filter_wide_kernel" in plan.kernel_name(vs.VS_KIND_SYNTH)
    narrow, _, _ = configs.wide_order_lanes([5, 22, 17])
    with engine.plan(narrow, 1000) as plan:
        assert "wide" not in plan.kernel_name(vs.VS_KIND_SYNTH)


def test_filter_only_kind_with_wide_sets(engine):
    lanes, fs, dur = _lanes(130)
    rng = np.random.default_rng(3)
    flow = rng.integers(-20000, 20000, size=(130, 7001), dtype=np.int16)
    assert np.array_equal(engine.filter(lanes, flow), po.filter(lanes, flow))


def test_fma_mode_distance_follows_the_conditioning_of_the_set(engine):
    """VS_ARITH_FMA rounds differently from the reference's mul-then-subtract; how far the int16 output
    can move depends on the SET: the reference's tables and sets with moderate coefficients stay
    within +-1 LSB, a direct form of order 40 with coefficients of 1e4 amplifies last-bit differences
    (its exact-double output is itself several LSB from a long-double evaluation).  Asserted: +-1 LSB
    wherever max |A[j]| <= 500, and a handful of samples at most elsewhere."""
    lanes, fs, dur = _lanes(200)
    n = 8000
    want = po.synth(lanes, n).astype(np.int32)
    engine.set_arith(vs.VS_ARITH_FMA)
    try:
        got = engine.synth(lanes, n).astype(np.int32)
    finally:
        engine.set_arith(vs.VS_ARITH_EXACT)
    d = np.abs(got - want)
    tame = np.array([np.abs(np.array(l.A[:])).max() <= 500 for l in lanes])
    assert tame.sum() > 150
    assert d[tame].max() <= 1
    assert np.count_nonzero(d) <= d.size // 100000


def test_tables_and_wide_sets_in_one_batch_with_output_noise(engine):
    """one wide lane makes the plan wide; table lanes, low-order sets and `vowel -n` noise ride along"""
    specs, fs, dur, _ = configs.config_specs(3, 150)
    plain, d = vs.lanes_from_specs(specs)
    wide, _, _ = _lanes(150)
    mixed = []
    for k in range(150):
        a, b = plain[k], wide[k]
        if k % 3 == 0:
            a.out_snr = 100.0
            b.out_snr = 31.6
        mixed += [a, b]
    n = 9000
    got = engine.synth(mixed, n)
    assert np.array_equal(got, po.synth(mixed, n))


def test_one_wide_lane_in_the_second_chunk_of_the_host_pipeline(engine):
    """vs_synth cuts the batch into chunks of 16384 utterances with a plan each: only the chunk that
    holds the wide lane takes the wide path"""
    specs, fs, dur, _ = configs.config_specs(3, 16384 + 40)
    lanes, d = vs.lanes_from_specs(specs)
    wide, _, _ = configs.wide_order_lanes([40])
    C.memmove(C.byref(lanes, (16384 + 7) * C.sizeof(vs.Lane)), C.byref(wide[0]), C.sizeof(vs.Lane))
    n = 3000
    got = engine.synth(lanes, n)
    pick = [0, 16383, 16384, 16384 + 6, 16384 + 7, 16384 + 8, 16384 + 39]
    assert np.array_equal(got[pick], po.synth([lanes[i] for i in pick], n))
    assert np.array_equal(got[16384:], po.synth([lanes[i] for i in range(16384, 16384 + 40)], n))


def test_unaligned_rows_take_the_scalar_path(engine):
    lanes, fs, dur = _lanes(70)
    n = 1001
    pitch = 1003                       # odd pitch: rows are not 4-byte aligned
    with engine.scope() as dev:
        buf = dev.room(70 * pitch * 2)
        with engine.plan(lanes, n) as plan:
            plan.launch(vs.VS_KIND_SYNTH, buf, out_pitch=pitch)
            plan.status()
        got = engine.dev_download(buf, (70, pitch))[:, :n]
    assert np.array_equal(got, po.synth(lanes, n))
