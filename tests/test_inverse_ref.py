"""The numpy restatement of the inverse filter (tests/inverse_ref.py, include/voice_synth.h "inverse filtering") on the
CPU: the header's consequences (a), (b) and (c); the round trip through the restatement of the coefficient tracks, within
the bound the header derives; the claim the feature is built for -- on inverse-filtered vowels the acoustic measure reads
the shimmer of the flow again; and the host helper vs_inverse_from_lpc.  The second half builds the hostile cases of
tests/test_gpu_inverse.py with the conditions under which those comparisons mean something, asserted from the restatement
alone.  The GPU tests compare the device with this restatement, which carries these checks over."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import _ffi
from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402
import inverse_ref as ir  # noqa: E402
import lpc_ref as lr  # noqa: E402
import track_ref as tr  # noqa: E402
from test_acoustic_ref import speech  # noqa: E402

TABLES = "aiu1234567"
# (pre-emphasis mu, gain g) of the round trips; the inverse runs de_emphasis = mu and scale = 1 / g
PAIRS = [(1.0, 0.25), (0.9, 0.1), (0.0, 0.02), (0.37, 0.05)]
ROUND_FS, ROUND_N = 16000, 16000
INT32 = 2.0 ** 31


def test_records_match_the_header():
    assert C.sizeof(_ffi.InverseRow) == 24 and vs.INVERSE_ROW_DTYPE.itemsize == 24 and ir.ROW_DTYPE.itemsize == 24
    assert C.sizeof(_ffi.InverseStat) == 16 and vs.INVERSE_STAT_DTYPE.itemsize == 16
    assert vs.INVERSE_ROW_DTYPE == ir.ROW_DTYPE and vs.INVERSE_STAT_DTYPE == ir.STAT_DTYPE
    assert vs.VS_INVERSE_NO_SET == 1 and ir.NO_SET == 1
    rows = vs.inverse_rows(3, 2, [5, 6, 7], -1, 100, 0.5, [0.0, 0.9, 1.0])
    assert rows.dtype == ir.ROW_DTYPE and list(rows["hop"]) == [5, 6, 7] and rows["scale"][2] == 0.5
    assert rows["de_emphasis"][1] == np.float32(0.9) and (rows["length"] == 100).all() and (rows["offset"] == -1).all()


# 1 ---- consequences (a) and (b)

def _noise_rows(rng, R, N):
    x = rng.integers(-32768, 32768, (R, N)).astype(np.int16)
    x[0, :40] = -32768
    x[1, ::3] = 32767
    return x


@pytest.mark.parametrize("arith", ["exact", "fma"])
def test_without_de_emphasis_u_is_the_input_and_zero_taps_copy_the_row(arith):
    rng = np.random.default_rng(1)
    R, N = 6, 300
    x = _noise_rows(rng, R, N)
    for order in (1, 22, 40):
        # (b): all taps 0, rho 0, scale 1: the row itself, -32768 -> -32767 and counted as clipped
        coefs = np.zeros((R, 2, order + 1))
        coefs[..., 0] = 1.0
        for mode in (ir.HOLD, ir.GLIDE):
            got, stat = ir.inverse_filter(x, coefs, ir.rows_of(R, 2, 70, 10, N), mode, arith=arith)
            assert np.array_equal(got, np.maximum(x, -32767)), (order, mode)
            assert np.array_equal(stat["n_clipped"], (x == -32768).sum(axis=1)) and stat["n_clipped"][0] >= 40
            assert not stat["status"].any() and not stat["n_unusable"].any() and not stat["reserved_"].any()
        # (a): rho 0: u = s exactly, so integer taps give the integer FIR sum exactly, in either arithmetic
        taps = rng.integers(-3, 4, (R, 1, order + 1)).astype(np.float64)
        want = x.astype(np.int64).copy()
        for j in range(1, order + 1):
            want[:, j:] += taps[:, 0, j].astype(np.int64)[:, None] * x[:, :N - j].astype(np.int64)
        ext = []
        got, stat = ir.inverse_filter(x, taps, ir.rows_of(R, 1, 1, 0, N, 0.5), ir.HOLD, arith=arith, extremes=ext)
        assert np.array_equal(got, tr.round2int(want * 0.5)), order
        assert ext[0][0].min() == (want * 0.5).min() and ext[0][1].max() == (want * 0.5).max()
        assert np.array_equal(stat["n_clipped"], ir.clipped(want * 0.5).sum(axis=1))


def test_samples_past_the_length_and_rows_without_a_set():
    rng = np.random.default_rng(2)
    x = _noise_rows(rng, 4, 100)
    coefs = np.zeros((4, 3, 5))
    coefs[1, :, 2] = np.nan
    coefs[2, 1, 4] = np.inf
    rows = ir.rows_of(4, 3, 20, 0, [100, 60, 0, 33])
    got, stat = ir.inverse_filter(x, coefs, rows, ir.HOLD, out=np.full((4, 100), 0x5A5A, dtype=np.int16))
    assert list(stat["status"]) == [0, ir.NO_SET, 0, 0] and list(stat["n_unusable"]) == [0, 3, 1, 0]
    assert not got[1, :60].any() and stat["n_clipped"][1] == 0
    for r in range(4):
        assert (got[r, rows["length"][r]:] == 0x5A5A).all()
    assert np.array_equal(got[3, :33], np.maximum(x[3, :33], -32767))


# 2 ---- consequence (c): the round trip through the coefficient tracks, one set held

def _pair_arrays(n):
    mu = np.array([PAIRS[r % 4][0] for r in range(n)], dtype=np.float32)
    g = np.array([PAIRS[r % 4][1] for r in range(n)], dtype=np.float32)
    return mu, g, (1.0 / g.astype(np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def round_trip_flows():
    """the oracle's flows of the round trips: ten tables x four rows, 16 kHz, 1 s, -f 90..120 -s 5 -j 1 -n 20"""
    lanes = []
    for k, v in enumerate(TABLES):
        for r in range(4):
            i = 4 * k + r
            lanes.append(vs.lane_from_cli(["-r", str(ROUND_FS), "-d", "1", "-f", str(90 + (30 * i) // 39), "-s", "5", "-j",
                                           "1", "-n", "20"], ["-v", v], 500 + i)[0])
    flow = pyoracle.source(lanes, ROUND_N)
    flow.setflags(write=False)
    return flow


def table_sets():
    """coefs [40][1][23]: the table of each row of round_trip_flows()"""
    return np.array([vs.vowel_coefficients(v) for v in TABLES]).repeat(4, axis=0)[:, None, :]


def hold_bounds():
    mu, g, scale = _pair_arrays(40)
    A = table_sets()[:, 0]
    return np.array([ir.round_trip_bound(A[r], mu[r], scale[r], ROUND_N) for r in range(40)])


def test_round_trip_through_a_held_table_stays_within_the_derived_bound():
    flow = round_trip_flows()
    coefs = table_sets()
    mu, g, scale = _pair_arrays(40)
    trows = np.zeros(40, dtype=tr.ROW_DTYPE)
    trows["n_sets"], trows["hop"], trows["length"], trows["gain"], trows["pre_emphasis"] = 1, 1, ROUND_N, g, mu
    pcm, tstat = tr.filter_track(flow, coefs, trows, tr.HOLD)
    peaks = np.abs(pcm.astype(np.int32)).reshape(10, 4, -1).max(axis=(0, 2))
    print("largest |sample| of the filtered rows per (mu, g) pair:", [int(v) for v in peaks])
    assert peaks.max() < 32767 and peaks.min() > 2000            # no sample clips, and none of the pairs is silent
    got, stat = ir.inverse_filter(pcm, coefs, ir.rows_of(40, 1, 1, 0, ROUND_N, scale, mu), ir.HOLD)
    assert not stat["status"].any() and not stat["n_clipped"].any()
    err = np.abs(got.astype(np.int32) - flow.astype(np.int32)).max(axis=1)
    bound = hold_bounds()
    for q in range(4):
        print("mu %.2f g %.2f: largest |inverse - flow| %s LSB, derived bounds %s" % (
            PAIRS[q][0], PAIRS[q][1], [int(v) for v in err[q::4]], [int(b) for b in bound[q::4]]))
    assert (err <= bound).all(), (err, bound)
    assert err.max() >= 1                                        # (the round trip is not an identity: something is measured)
    # the FMA form on a prefix of every fifth row (a prefix of the inverse is the inverse of the prefix)
    sel, n = np.arange(0, 40, 5), 3000
    fma, _ = ir.inverse_filter(pcm[sel, :n], coefs[sel], ir.rows_of(len(sel), 1, 1, 0, n, scale[sel], mu[sel]), ir.HOLD,
                               arith="fma")
    d = np.abs(fma.astype(np.int32) - got[sel, :n].astype(np.int32)).max()
    print("FMA form against the exact form on the prefixes: at most %d LSB" % d)
    assert d <= 1


# 3 ---- the same round trip through a glide

GLIDE_PAIRS = [("a", "i"), ("u", "a"), ("1", "7")]


def test_round_trip_through_a_glide_stays_small():
    """101 anchors at hop 160 from one table to another, so the set changes in every group of the row; asserted: the
    error stays within twice the larger derived bound of the two end tables"""
    flow = round_trip_flows()[:12]
    mu, g, scale = _pair_arrays(12)
    coefs = np.array([tr.glide_sets(vs.vowel_coefficients(a), vs.vowel_coefficients(b), 101) for a, b in GLIDE_PAIRS])
    coefs = coefs.repeat(4, axis=0)
    trows = np.zeros(12, dtype=tr.ROW_DTYPE)
    trows["n_sets"], trows["hop"], trows["length"], trows["gain"], trows["pre_emphasis"] = 101, 160, ROUND_N, g, mu
    pcm, tstat = tr.filter_track(flow, coefs, trows, tr.GLIDE)
    assert np.abs(pcm.astype(np.int32)).max() < 32767 and not tstat["n_unusable"].any()
    got, stat = ir.inverse_filter(pcm, coefs, ir.rows_of(12, 101, 160, 0, ROUND_N, scale, mu), ir.GLIDE)
    assert not stat["status"].any() and not stat["n_unusable"].any() and not stat["n_clipped"].any()
    err = np.abs(got.astype(np.int32) - flow.astype(np.int32)).max(axis=1)
    bound = np.array([2 * max(ir.round_trip_bound(coefs[r, 0], mu[r], scale[r], ROUND_N),
                              ir.round_trip_bound(coefs[r, -1], mu[r], scale[r], ROUND_N)) for r in range(12)])
    print("glides: largest |inverse - flow| %s LSB, twice the larger end bound %s" % ([int(v) for v in err], [int(b) for b in bound]))
    assert (err <= bound).all(), (err, bound)


# 4 ---- what the feature is for: the source's shimmer read from speech

@pytest.mark.parametrize("S", [2, 5, 10])
def test_inverse_filtered_vowels_read_the_shimmer_of_the_flow(S):
    """the CPU oracle's vowels of tests/test_acoustic_ref.py (-v a, gain 10, pre-emphasis 1, 22050 Hz, F0 100), 16 rows:
    the known table with rho = 1 and scale 1/10 gives the flow's mean shimmer back within 0.001 (measured gap <= 0.0001),
    where the speech itself reads more than 0.004 below it"""
    lanes, ns, pcm = speech(["-s", str(S)], [], 300, n=16)
    flow = pyoracle.source(lanes, ns)
    coefs = np.broadcast_to(vs.vowel_coefficients("a"), (16, 1, 23))
    inv, stat = ir.inverse_filter(pcm, coefs, ir.rows_of(16, 1, 1, 0, ns, 1.0 / lanes[0].gain, lanes[0].pre_emphasis),
                                  ir.HOLD)
    assert lanes[0].gain == 10.0 and lanes[0].pre_emphasis == 1.0 and not stat["status"].any()
    on_flow, on_speech, on_inverse = (ar.measure(x, 22050)["shimmer_local"].mean() for x in (flow, pcm, inv))
    print("set shimmer %d %%: on the flow %.4f, on the speech %.4f, on the inverse-filtered speech %.4f; %d samples of "
          "the speech at the clamp" % (S, on_flow, on_speech, on_inverse, int((np.abs(pcm.astype(np.int32)) >= 32767).sum())))
    assert abs(on_inverse - on_flow) <= 0.001
    assert abs(on_speech - on_flow) > 0.004


# 6 ---- the host helper

def test_inverse_rows_from_lpc_options():
    """the option grid of tests/test_track_ref.py's rows, in both modes"""
    rng = np.random.default_rng(5)
    made = refused = 0
    for _ in range(1500):
        fs = int(rng.choice([8000, 11025, 16000, 22050, 44100, 48000, 96000, int(rng.integers(1000, 200000))]))
        o = lr.opts(order=int(rng.integers(1, 41)), window=int(rng.integers(0, 2)),
                    window_s=float(rng.choice([0.005, 0.02, 0.025, 0.04, rng.uniform(0.0005, 0.4)])),
                    hop_s=float(rng.choice([0.0, 0.005, 0.01, rng.uniform(0.0, 0.05)])),
                    pre_emphasis=int(rng.integers(0, 2)), n_formants=int(rng.integers(0, 21)))
        length = int(rng.integers(0, 40000))
        plan = lr.frame_plan(fs, length, o)
        for mode, name in ((ir.HOLD, "hold"), (ir.GLIDE, "glide")):
            want = None if plan is None else ir.from_lpc(plan[0], plan[1], o["pre_emphasis"], len(plan[2]), length, mode)
            if want is None:
                with pytest.raises(vs.VsError):
                    vs.inverse_from_lpc(fs, length, name, **o)
                refused += 1
            else:
                got = vs.inverse_from_lpc(fs, length, name, **o)
                assert tuple(got) == want, (fs, length, o, mode)
                assert tuple(got)[:4] == tuple(vs.track_from_lpc(fs, length, name, **o))[:4]
                made += 1
    assert made > 500 and refused > 50
    assert tuple(vs.inverse_from_lpc(16000, 16000, "glide")) == (98, 160, 200, 16000, 1.0, 0.0)
    assert vs.inverse_from_lpc(16000, 16000, "hold")["offset"] == 120
    row = _ffi.InverseRow()
    assert vs.load().vs_inverse_from_lpc(None, 16000, 16000, 0, None) == _ffi.VS_ERR_ARG
    assert vs.load().vs_inverse_from_lpc(None, 16000, 16000, 7, C.byref(row)) == _ffi.VS_ERR_ARG
    assert vs.load().vs_inverse_from_lpc(None, 16000, 16000, 1, C.byref(row)) == 0 and row.offset == 200


# 5 ---- the hostile cases of tests/test_gpu_inverse.py ------------------------------------------------------------------

HOSTILE_N = 1210          # 50 groups of 24, one whole vector of 8 and two scalar samples
HOSTILE_ORDERS = (1, 12, 22, 23, 40)
SENTINEL = 0x5A5A


def _ints(a):
    return [int(v) for v in a]


class Case(dict):
    """the inputs of one comparison and what the restatement makes of them: pcm, coefs, rows, mode, out, want =
    (flow, stat), lo / hi (ir.inverse_filter's extremes, per row)"""
    __getattr__ = dict.__getitem__


def restated(pcm, coefs, rows, mode, out=None, arith="exact"):
    ext = []
    want = ir.inverse_filter(pcm, coefs, rows, mode, out=out, arith=arith, extremes=ext)
    for a in want:
        a.setflags(write=False)
    return Case(pcm=pcm, coefs=coefs, rows=rows, mode=mode, out=out, want=want, lo=ext[0][0], hi=ext[0][1])


def _alternating(R, N):
    x = np.where(np.arange(N) % 2 == 0, 32767, -32768).astype(np.int16)
    return np.tile(x, (R, 1))


@functools.lru_cache(maxsize=None)
def saturation_case(order, arith="exact"):
    """full-scale alternating input on taps of alternating sign, so that every product has the sign of s[n]: integer
    taps, rho 0 and scales that are powers of two, hence e*c is an integer computed without any rounding, and n_clipped
    can be counted in integer arithmetic.  Row r: tap size 4^r, scale 2^(r % 4 - 1); rows 12..15 shorter than the rest;
    rows 0..3 alternate between +-300 only, so that not every row clips at every sample."""
    R, N = 16, HOSTILE_N
    pcm = _alternating(R, N)
    pcm[:4] = np.where(pcm[:4] > 0, 300, -300)
    size = 4.0 ** np.arange(R)
    coefs = np.zeros((R, 1, order + 1))
    coefs[:, 0, 0] = 1.0
    coefs[:, 0, 1:] = size[:, None] * np.where(np.arange(1, order + 1) % 2 == 1, -1.0, 1.0)[None, :]
    scale = 2.0 ** (np.arange(R) % 4 - 1)
    length = np.where(np.arange(R) >= 12, N - 37 * (np.arange(R) - 11), N)
    return restated(pcm, coefs, ir.rows_of(R, 1, 1, 0, length, scale, 0.0), ir.HOLD, arith=arith,
                    out=np.full((R, N), SENTINEL, dtype=np.int16))


def check_saturation_conditions(order):
    """returns the line for the profile"""
    c = saturation_case(order)
    R, N = c.pcm.shape
    # the same sums in Python integers
    want_clipped = np.zeros(R, dtype=np.int64)
    for r in range(R):
        taps = [int(v) for v in c.coefs[r, 0]]
        s = [int(v) for v in c.pcm[r]]
        num, den = (int(c.rows["scale"][r]), 1) if c.rows["scale"][r] >= 1 else (1, 2)
        for n in range(int(c.rows["length"][r])):
            e = s[n] + sum(taps[j] * s[n - j] for j in range(1, min(order, n) + 1))
            assert abs(e * num) < 2 ** 53
            v = (e * num) // den if (e * num) % den == 0 else None     # x.5: round2int floors it (dec is not > 0.5)
            if v is None:
                v = (e * num - 1) // den
            want_clipped[r] += (v > 32767 or v < -32767)
    assert np.array_equal(c.want[1]["n_clipped"], want_clipped), (c.want[1]["n_clipped"], want_clipped)
    assert c.lo.min() < -INT32 and c.hi.max() > INT32, (c.lo.min(), c.hi.max())
    assert (want_clipped < N).any() and (want_clipped == N).any()         # some rows partly, some at every sample
    assert np.isfinite(c.lo).all() and np.isfinite(c.hi).all()
    for r in range(R):
        assert (c.want[0][r, c.rows["length"][r]:] == SENTINEL).all()
    fma = saturation_case(order, "fma")
    assert np.array_equal(fma.want[0], c.want[0]) and np.array_equal(fma.want[1], c.want[1])   # nothing rounds
    return "order %2d: e*c in [%.3e, %.3e], n_clipped %s" % (order, c.lo.min(), c.hi.max(), _ints(want_clipped))


@pytest.mark.parametrize("order", HOSTILE_ORDERS)
def test_saturation_cases_pass_int32_in_both_signs_with_an_exact_count(order):
    print(check_saturation_conditions(order))


@functools.lru_cache(maxsize=None)
def integrator_case(order, mode, arith="exact"):
    """rho = 1 on constant rows of -32768 (and one of 32767, one of zeros): u[n] = -32768 (n + 1), every value exact;
    the ten tables (orders other than 22: their first reflection coefficients, or more small ones)"""
    R, N = 12, HOSTILE_N
    pcm = np.full((R, N), -32768, dtype=np.int16)
    pcm[10], pcm[11] = 32767, 0
    coefs = table_like_sets(np.random.default_rng(order), R, 2, order)
    scale = np.array([1.0, 0.5, 0.01, 8.0] * 3)
    return restated(pcm, coefs, ir.rows_of(R, 2, 500, 100, N, scale, 1.0), mode, arith=arith)


def table_like_sets(rng, R, K, order):
    """[R][K][order+1]: blends of the ten tables in the reflection domain (tests/test_gpu_track.py's _blend_sets)"""
    kt = np.array([tr.reflection(vs.vowel_coefficients(v))[0] for v in TABLES])
    a, b = rng.integers(0, 10, (R, K)), rng.integers(0, 10, (R, K))
    w = rng.uniform(0, 1, (R, K, 1))
    k = w * kt[a] + (1.0 - w) * kt[b]
    if order <= 22:
        k = k[..., :order]
    else:
        k = np.concatenate([k, rng.uniform(-0.2, 0.2, (R, K, order - 22))], axis=-1)
    return tr.step_up(k)


def test_integrator_on_a_constant_full_scale_row():
    for order in (22, 40):
        c = integrator_case(order, ir.HOLD)
        # A(1) of a vowel table is small but not zero: the ramp -32768 (n + 1) A(1) leaves int16 on the loud rows
        assert c.want[1]["n_clipped"].max() > HOSTILE_N // 2 and not c.want[1]["status"].any()
        assert not c.want[0][11].any() and c.want[1]["n_clipped"][11] == 0
        assert np.isfinite(c.lo).all() and np.isfinite(c.hi).all()
        print("order %d: rho = 1 on constant rows: e*c in [%.3e, %.3e], n_clipped %s" % (
            order, c.lo.min(), c.hi.max(), _ints(c.want[1]["n_clipped"])))


@functools.lru_cache(maxsize=None)
def unusable_case(order, mode, arith="exact"):
    """NaN sets at the start, in the middle and at the end; rows without any usable set; sets that only a glide refuses
    (finite, |k_p| >= 1); sets beyond n_sets that do not count.  Noise input, rho and scale drawn."""
    R, N, K = 16, HOSTILE_N, 9
    rng = np.random.default_rng(100 + order)
    pcm = rng.integers(-32768, 32768, (R, N)).astype(np.int16)
    coefs = table_like_sets(rng, R, K, order)
    coefs[0, :3, 1:] = np.nan                    # at the start: E_0..E_2 are the first usable set
    coefs[1, 4, 1 + (7 % order)] = np.nan        # in the middle
    coefs[2, K - 1, 1] = np.inf                  # at the end
    coefs[3, :, order] = np.nan                  # no usable set at all
    coefs[4, 2:7, 1 + (3 % order)] = np.nan
    coefs[5, :, 1:] = np.nan                     # all NaN
    coefs[6, 0, 1:] = np.nan
    coefs[6, 5, 1:] = np.nan
    coefs[7, 2] = np.concatenate([[1.0], np.zeros(order - 1), [1.25]])   # finite, |k_p| >= 1: unusable in a glide only
    coefs[8, :, 1:] = 0.0
    coefs[8, :, order] = np.where(np.arange(K) % 2, 1.0, -1.0)           # ... in every set: NO_SET in a glide
    coefs[9, 3:, 1 + (5 % order)] = np.nan       # beyond n_sets: not counted
    rows = ir.rows_of(R, K, 130, 40, N, rng.uniform(0.1, 2.0, R), rng.choice([0.0, 0.37, 0.9, 1.0], R))
    rows["n_sets"][9] = 3
    rows["length"] = np.where(np.arange(R) % 2, N, N - 77 * np.arange(R))
    rows["hop"][10], rows["offset"][10] = 1, -5  # every set behind the first group: tested behind the walk
    coefs[10, 6, 1] = np.nan
    rows["hop"][11] = 5000                       # the row ends inside set 0: the others are tested behind the last sample
    coefs[11, 7, 1] = np.nan
    return restated(pcm, coefs, rows, mode, arith=arith, out=np.full((R, N), SENTINEL, dtype=np.int16))


@pytest.mark.parametrize("order", HOSTILE_ORDERS)
def test_unusable_sets_in_the_restatement(order):
    for mode in (ir.HOLD, ir.GLIDE):
        c = unusable_case(order, mode)
        st = c.want[1]
        glide = mode == ir.GLIDE
        K = 9
        assert list(st["n_unusable"][:7]) == [3, 1, 1, K, 5, K, 2] and st["n_unusable"][9] == 0
        assert st["n_unusable"][7] == (1 if glide else 0) and st["n_unusable"][8] == (K if glide else 0)
        assert st["n_unusable"][10] == 1 and st["n_unusable"][11] == 1
        none = [3, 5] + ([8] if glide else [])
        assert [r for r in range(16) if st["status"][r]] == none
        for r in range(16):
            n = c.rows["length"][r]
            assert (c.want[0][r, n:] == SENTINEL).all()
            if r in none:
                assert not c.want[0][r, :n].any() and st["n_clipped"][r] == 0
        assert np.isfinite(c.lo[st["status"] == 0]).all()


CANCEL_ORDERS = (12, 22, 23, 40)


@functools.lru_cache(maxsize=None)
def cancelling_case(order, arith):
    """taps +-B in turn with B about 1e12 plus a small part, on rows that are constant for 100 samples at a time: in a
    constant stretch the big products cancel, and what is left shows how they were rounded -- one by one (a step of 2
    at 1e16) or inside an fma.  Hold mode runs such taps as they are.  On integer-valued, well-scaled sets the two forms
    give the same bytes, so a device that ran the wrong form would pass everywhere else."""
    R, N = 8, HOSTILE_N
    rng = np.random.default_rng(700 + order)
    pcm = (rng.integers(-20000, 20000, (R, N // 100 + 1)).repeat(100, axis=1)[:, :N]).astype(np.int16)
    B = 1e12 * rng.uniform(1, 2, (R, 1, order // 2))
    coefs = np.zeros((R, 1, order + 1))
    coefs[..., 0] = 1.0
    coefs[..., 1:2 * (order // 2):2] = B
    coefs[..., 2:2 * (order // 2) + 1:2] = -B
    coefs[..., 1:] += rng.uniform(-0.1, 0.1, (R, 1, order))
    return restated(pcm, coefs, ir.rows_of(R, 1, 1, 0, N, rng.uniform(0.1, 1.0, R), 0.0), ir.HOLD, arith=arith)


@pytest.mark.parametrize("order", CANCEL_ORDERS)
def test_cancelling_taps_tell_the_two_arithmetics_apart(order):
    e, f = cancelling_case(order, "exact"), cancelling_case(order, "fma")
    differ = (e.want[0] != f.want[0]).mean()
    quiet = (np.abs(f.want[0].astype(np.int32)) < 32767).mean()
    print("order %d: the forms differ in %.1f %% of the samples; %.1f %% of the FMA form's lie inside the clamp" % (
        order, 100 * differ, 100 * quiet))
    assert differ > 0.25 and quiet > 0.5
