"""The coefficient-track kernels (csrc/vs_track.hip) on what tests/test_gpu_track.py never feeds them, byte for byte
against the numpy restatement (tests/track_ref.py), PCM and status records:

  a. sets that take the filter past int32 in both signs (the clamp sits behind the conversion on the device);
  b. the same clamp in vs_filter, on the fused kernels (both instantiations) and on the wide kernel;
  c. unstable sets, which hold mode runs and glide mode refuses;
  d. odd pitches and base pointers that are only 2-byte aligned through vs_track_launch (the scalar load/store path),
     with the padding and the samples past a row's length left alone;
  e. rows shorter than one pass of 24 or 48 samples and partial last wavefronts;
  f. the FMA form against the restatement's FMA form (VS_ARITH_F32 runs it too; hold with one set is vs_filter's);
  g. the sets vs_lpc makes of recordings: constants, tones, noise, and silence at the start, the middle and the end.

The cases and the conditions under which they mean something (how far past int32, how many samples saturate) are built
and asserted on the CPU in tests/test_track_ref.py; here the device runs them.  Every test prints what it measured
(pytest -s): profiles/track_hostile_signals.txt keeps those lines."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_signals as hs  # noqa: E402
import test_track_ref as cases  # noqa: E402
import track_ref as tr  # noqa: E402
from test_track_ref import HOSTILE_N as N  # noqa: E402
from gpu_support import INPUT_PAD, SENTINEL, GuardedRows  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [tr.HOLD, tr.GLIDE]
MODE_NAME = {tr.HOLD: "hold", tr.GLIDE: "glide"}


def _device(engine, c, rows=None, out=None):
    """vs_track on a case (or on its first `rows` rows)"""
    n = len(c.rows) if rows is None else rows
    r = c.rows[:n]
    return engine.filter_track(c.flow[:n], c.coefs[:n], r["hop"], r["offset"], r["n_sets"], r["length"], r["gain"],
                               r["pre_emphasis"], MODE_NAME[c.mode], None if c.gains is None else c.gains[:n],
                               None if out is None else out[:n])


def _assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:8])
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:8])


# a ---- saturation past int32, both signs

@pytest.mark.parametrize("with_gains", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", cases.SAT_ORDERS)
def test_saturation_past_int32(engine, order, mode, with_gains):
    line = cases.check_saturation_conditions(order, mode)
    c = cases.saturation_case(order, mode, with_gains)
    _assert_same(_device(engine, c), c.want)
    if with_gains:
        print(line)


# b ---- the same clamp in vs_filter

@pytest.mark.parametrize("kind", cases.CLAMP_KINDS)
def test_filter_clamps_past_int32(engine, kind):
    c = cases.clamp_case(kind)
    assert c.state_max < cases.STATE_FINITE and c.lo.min() < -cases.INT32 and c.hi.max() > cases.INT32
    want = pyoracle.filter(c.lanes, c.flow)
    assert np.array_equal(want, c.want[0])
    with engine.plan(c.lanes, N) as plan:
        name = plan.kernel_name(vs.VS_KIND_FILTER)
    assert ("vs_filter_wide_kernel" in name) == (kind == "wide")
    assert ("false, true>" in name) == (kind == "tables_pre1"), name      # the pre-emphasis-1.0 instantiation
    got = engine.filter(c.lanes, c.flow)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    _assert_same(_device(engine, c), c.want)
    print("vs_filter %-11s %s: %d lanes, saturated %.1f %%, o in [%.3e, %.3e]" % (
        kind, name, len(c.lanes), 100 * cases.saturated(want).mean(), c.lo.min(), c.hi.max()))


# c ---- hold runs unstable sets, glide refuses them

def test_hold_runs_unstable_sets(engine):
    c = cases.unstable_case(tr.HOLD)
    assert c.state_max < cases.STATE_FINITE and not c.want[1]["status"].any()
    _assert_same(_device(engine, c, out=np.full(c.flow.shape, SENTINEL, dtype=np.int16)), c.want)
    print("unstable sets (largest root radius %.2f) in hold mode: max |y| %.3e, saturated %.1f %%" % (
        cases.UNSTABLE_RADIUS, c.state_max, 100 * cases.saturated(c.want[0]).mean()))


def test_glide_refuses_unstable_sets(engine):
    c = cases.unstable_case(tr.GLIDE)
    got = _device(engine, c, out=np.full(c.flow.shape, SENTINEL, dtype=np.int16))
    _assert_same(got, c.want)
    assert (got[1]["status"] == vs.VS_TRACK_NO_SET).all() and (got[1]["n_unusable"] == 3).all()
    for r, n in enumerate(c.rows["length"]):
        assert not got[0][r, :n].any() and (got[0][r, n:] == SENTINEL).all()


# d ---- layouts through vs_track_launch

LAYOUTS = [(N, N), (N + 1, N), (N, N + 1), (N + 6, N + 3)]
BASES = [(0, 0), (2, 0), (0, 2), (2, 2)]        # bytes added to the (256-byte aligned) allocations of flow and output


def _layout_case(order, mode):
    R = 70                                      # a whole wavefront and a partial one
    rng = np.random.default_rng(400 + order)
    coefs = hs.reflection_sets(rng, R, 4, order)
    rows = np.zeros(R, dtype=tr.ROW_DTYPE)
    rows["n_sets"], rows["hop"], rows["offset"] = 4, 300, rng.integers(-30, 30, R)
    rows["length"] = rng.integers(0, N + 1, R)
    rows["length"][:6] = [N, 0, N - 1, 1, 8, N - 8]
    rows["gain"], rows["pre_emphasis"] = rng.choice([1.0, 8.0], R), rng.choice([0.0, 0.9, 1.0], R)
    flow = cases.hostile_flows()[1][np.arange(R) % 17]
    return cases.restated(flow, coefs, rows, mode, out=np.full((R, N), SENTINEL, dtype=np.int16))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [22, 40])
def test_pitches_and_alignments_through_the_launch(engine, order, mode):
    c = _layout_case(order, mode)
    assert c.state_max < cases.STATE_FINITE
    R = len(c.rows)
    with engine.scope() as dev:
        cf_d, st_d = dev.put(c.coefs), dev.room(R * 8)
        out = GuardedRows(R, N, N + 6, 2).on(dev)
        in_d = dev.room(out.room * 2)
        for in_pitch, out_pitch in LAYOUTS:
            for in_off, out_off in BASES:
                what = (in_pitch, out_pitch, in_off, out_off)
                staged = np.full((R, in_pitch), INPUT_PAD, dtype=np.int16)      # the padding of the flow is not silence
                staged[:, :N] = c.flow
                engine.dev_upload(in_d + in_off, staged)
                out.fill()
                engine.dev_upload(st_d, np.full(R, -1, dtype=vs.TRACK_STAT_DTYPE))
                engine.filter_track_dev(MODE_NAME[mode], order, in_d + in_off, in_pitch, out.first(out_pitch, out_off),
                                        out_pitch, R, N, c.rows, cf_d, 4, stat_ptr=st_d)
                engine.synchronize()
                body = out.rows_back(out_pitch, out_off, what)          # guards and pitch padding untouched
                _assert_same((body, dev.get(st_d, (R,), vs.TRACK_STAT_DTYPE)), c.want, what)


# e ---- short rows and partial wavefronts

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [22, 40])
def test_short_rows_and_partial_wavefronts(engine, order, mode):
    R, K = 129, 4
    rng = np.random.default_rng(500 + order)
    coefs = hs.reflection_sets(rng, R, K, order)
    gains = rng.uniform(0.25, 2.0, (R, K))
    bank = cases.hostile_flows()[1]
    for ns in (1, 7, 8, 9, 23, 24, 25, 47, 48, 49):
        for hop in (1, 24):
            rows = np.zeros(R, dtype=tr.ROW_DTYPE)
            rows["n_sets"], rows["hop"], rows["offset"] = K, hop, rng.integers(-2, 3, R)
            rows["length"] = rng.integers(0, ns + 1, R)
            rows["length"][[0, 62, 63, 64, 128]] = ns
            rows["gain"], rows["pre_emphasis"] = rng.choice([1.0, 64.0], R), rng.choice([0.0, 0.9, 1.0], R)
            start = rng.integers(0, N - ns, R)
            flow = np.stack([bank[r % 17, s:s + ns] for r, s in enumerate(start)])
            out = np.full((R, ns), SENTINEL, dtype=np.int16)
            c = cases.restated(flow, coefs, rows, mode, gains if hop == 24 else None, out=out)
            assert c.state_max < cases.STATE_FINITE
            for lanes in (1, 63, 65, 129):
                _assert_same(_device(engine, c, rows=lanes, out=out), (c.want[0][:lanes], c.want[1][:lanes]),
                             (ns, hop, lanes))


# f ---- the FMA form, byte for byte

# On the reflection-drawn sets the two arithmetics give the same PCM (a last-bit difference in y rarely crosses a
# rounding boundary of the int16 output), so a device that ran the exact form in VS_ARITH_FMA would pass there.  Sets
# with clustered poles are ill-conditioned enough to tell the forms apart: order // 2 pole pairs of radius r at angles
# within +-spread of one another (taps up to 1e6); there the forms differ in many samples, by up to hundreds of LSB.
CLUSTERS = {12: (0.99, 0.005), 22: (0.9, 0.1), 23: (0.9, 0.1), 40: (0.7, 0.3)}


def _clustered_set(order, rng):
    r, spread = CLUSTERS[order]
    centre = rng.uniform(1.0, 2.1)
    poles = []
    for _ in range(order // 2):
        z = r * np.exp(1j * (centre + rng.uniform(-spread, spread)))
        poles += [z, np.conj(z)]
    if order % 2:
        poles.append(rng.uniform(-0.5, 0.5))
    A = np.real(np.poly(poles))
    A[0] = 1.0
    return A


def _fma_case(order, mode, with_gains):
    """51 rows: the bank at row gain 1 and at row gain 64 on five reflection-drawn sets per row, and the bank on five
    clustered sets per row, at the row gain that takes the exact restatement's peak to 20000 (no saturation).  Returns
    the case (the FMA restatement) and the samples in which the exact restatement differs from it."""
    R, K = 51, cases.SAT_K
    rng = np.random.default_rng(600 + order)
    coefs = hs.reflection_sets(rng, R, K, order)
    coefs[34:] = [[_clustered_set(order, rng) for _ in range(K)] for _ in range(17)]
    gains = rng.uniform(0.25, 2.0, (R, K)) if with_gains else None
    rows = np.zeros(R, dtype=tr.ROW_DTYPE)
    rows["n_sets"], rows["length"] = K, N
    rows["hop"], rows["offset"] = rng.choice([23, 24, 25, 211], R), rng.choice([-17, 0, 24, 1000], R)
    rows["gain"], rows["pre_emphasis"] = np.where(np.arange(R) < 17, 1.0, 64.0), rng.choice([0.0, 0.9, 1.0], R)
    rows["gain"][34:] = 1.0
    flow = np.tile(cases.hostile_flows()[1], (3, 1))
    first = cases.restated(flow[34:], coefs[34:], rows[34:], mode, None if gains is None else gains[34:])
    rows["gain"][34:] = 20000.0 / np.maximum(np.maximum(-first.lo, first.hi), 1.0)
    exact = cases.restated(flow, coefs, rows, mode, gains)
    c = cases.restated(flow, coefs, rows, mode, gains, arith="fma")
    assert not c.want[1]["status"].any() and not c.want[1]["n_unusable"].any()
    return c, c.want[0] != exact.want[0]


@pytest.mark.parametrize("with_gains", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [12, 22, 23, 40])
def test_fma_form_equals_its_restatement(engine, order, mode, with_gains):
    c, differs = _fma_case(order, mode, with_gains)
    assert c.state_max < cases.STATE_FINITE
    assert differs.sum() >= 10 and differs.any(axis=1).sum() >= 3      # the forms can be told apart, on several rows
    exact = _device(engine, c)
    try:
        engine.set_arith(vs.VS_ARITH_FMA)
        fused = _device(engine, c)
        engine.set_arith(vs.VS_ARITH_F32)
        single = _device(engine, c)
    finally:
        engine.set_arith(vs.VS_ARITH_EXACT)
    _assert_same(fused, c.want)
    _assert_same(single, fused)                  # no single-precision form: VS_ARITH_F32 runs the FMA form
    d = np.abs(fused[0].astype(np.int32) - exact[0].astype(np.int32))
    assert np.array_equal(d > 0, differs)        # (implied by the two comparisons with the restatement's two forms)
    print("order %2d %-5s %s: FMA differs from exact in %d of %d samples on %d rows (%d by more than 1 LSB, at most %d "
          "LSB), saturated %.1f %%" % (order, MODE_NAME[mode], "per-set gains" if with_gains else "no gains     ",
                                       (d > 0).sum(), d.size, differs.any(axis=1).sum(), (d > 1).sum(), d.max(),
                                       100 * cases.saturated(c.want[0]).mean()))


def test_fma_hold_with_one_set_is_vs_filter(engine):
    c = cases.clamp_case("wide", "fma")
    try:
        engine.set_arith(vs.VS_ARITH_FMA)
        want = engine.filter(c.lanes, c.flow)
        got = _device(engine, c)
    finally:
        engine.set_arith(vs.VS_ARITH_EXACT)
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:8]
    _assert_same(got, c.want)
    exact = cases.clamp_case("wide").want[0]
    print("vs_filter wide under FMA: differs from exact in %d of %d samples" % ((want != exact).sum(), want.size))


# g ---- sets from recordings

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [12, 22, 40])
def test_sets_from_recordings(engine, order, mode):
    names, models, flow = cases.recording_inputs()
    coefs = engine.lpc(models, cases.HOSTILE_FS, coefs=True, order=order, **cases.RECORDING_OPTS)["coefs"]
    row = vs.track_from_lpc(cases.HOSTILE_FS, cases.RECORDING_N, MODE_NAME[mode], order=order, **cases.RECORDING_OPTS)
    assert row["n_sets"] == coefs.shape[1]
    c = cases.recording_case(order, mode)
    assert tuple(row) == tuple(c.rows[0])
    if not np.array_equal(coefs, c.coefs, equal_nan=True):       # (tests/test_gpu_lpc.py holds the device to them)
        c = cases.restated(flow, coefs, c.rows, mode)
    line = cases.check_recording_conditions(c)
    got = engine.filter_track(flow, coefs, row["hop"], row["offset"], mode=MODE_NAME[mode])
    _assert_same(got, c.want)
    assert got[1]["status"][names.index("zeros")] == vs.VS_TRACK_NO_SET
    assert np.array_equal(got[1]["n_unusable"], np.isnan(coefs[:, :, 1:]).any(axis=2).sum(axis=1))
    print("order %d %s: %s" % (order, MODE_NAME[mode], line))
