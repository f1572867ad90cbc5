"""The conditions under which the GPU tests on the hostile signal bank (tests/hostile_signals.py) mean something, shown on
the CPU with the numpy restatements alone: the bank drives the period kernel into its LDS opt-in, the second pass of its
lag-group loop and both ends of its k segmentation; it produces every status; it makes the marks kernel walk a stretch
again; it marks -32768; and it takes the LPC autocorrelation to half of int64's range.

If a condition fails after a change to the bank, it is the bank that has to change."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402
import hostile_signals as hs  # noqa: E402
import lpc_ref as lr  # noqa: E402


def lds_doubles(tmin, tmax):
    """vs_ac_xs_doubles, vs_ac_rp_doubles and vs_ac_lds_doubles of csrc/vs_acoustic.h, restated: (doubles of dynamic
    LDS of the period kernel, lag groups G, k segments S)"""
    xs = ((3 * tmax + 2 + 4) + 3) & ~3
    nl = tmax + 3 - tmin
    G = (nl + 3) // 4
    S = 1 if G >= 256 else 256 // G
    return xs + 4 * G * S + 8, G, S


@functools.lru_cache(maxsize=None)
def measured(case, polarity):
    """{name: (record, all marks, walk-again count, marked samples)} of one case under one polarity"""
    fs, n, f0_min, f0_max = case
    tmin, tmax = ar.lag_bounds(fs, f0_min, f0_max)
    out = {}
    for name, x in hs.bank(fs, n, 0).items():
        rec, m = ar.measure_row(x, fs, f0_min, f0_max, polarity, marks_pitch=10 ** 6)
        out[name] = (rec, m, hs.walk_again_marks(m, rec["p0"], tmin, tmax) if m else 0, [int(x[k]) for k in m[1:]])
    return out


def test_the_bank_is_deterministic_int16():
    a, b = hs.bank(16000, 8000, 5), hs.bank(16000, 8000, 5)
    assert list(a) == list(b) and len(a) >= 15
    for k in a:
        assert a[k].dtype == np.int16 and a[k].shape == (8000,) and np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["noise_full"], hs.bank(16000, 8000, 6)["noise_full"])
    assert a["noise_full"].min() < -32000 and a["noise_full"].max() > 32000
    assert a["noise_small"].min() == -3 and a["noise_small"].max() == 3
    assert (a["constant_min"] == -32768).all() and (a["constant"] == a["constant"][0]).all() and a["constant"][0] > 0
    assert set(np.unique(a["square_200"])) == {-32768, 32767} == set(np.unique(a["alternating"]))
    assert a["ramp"][0] == -32768 and a["ramp"][-1] == 32767
    names, m = hs.matrix(a)
    assert m.shape == (len(a), 8000) and m.dtype == np.int16 and names == list(a)


def test_cases_take_every_path_of_the_period_kernel():
    plan = {}
    for fs, n, f0_min, f0_max in hs.ACOUSTIC_CASES:
        tmin, tmax = ar.lag_bounds(fs, f0_min, f0_max)
        assert n >= 3 * tmax + 2
        plan[fs] = lds_doubles(tmin, tmax)
    assert plan[96000][0] == 8000 and 8 * plan[96000][0] > 48 * 1024   # the LDS opt-in
    for fs in (96000, 44100):                                         # a second pass of the lag-group loop
        assert plan[fs][1] > 256 and plan[fs][2] == 1
    assert 8 * plan[44100][0] <= 48 * 1024
    assert 1 < plan[16000][2] < 4
    assert plan[8000][2] > 20
    assert ar.lag_bounds(96000, 47.0, 500.0)[1] <= ar.AC_MAX_LAG


@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("case", hs.ACOUSTIC_CASES)
def test_acoustic_conditions(case, polarity):
    res = measured(case, polarity)
    status = {k: v[0]["status"] for k, v in res.items()}
    assert 0 in status.values()
    for k in hs.UNVOICED_ROWS:
        assert status[k] == ar.AC_UNVOICED, k
    for k in hs.ZERO_AMPLITUDE_ROWS:
        assert status[k] == ar.AC_ZERO_AMPLITUDE, k
    # a constant row has no local peak of r: P0 falls back to the first lag with r == rmax, the shortest
    assert res["constant"][0]["p0"] == ar.lag_bounds(case[0], case[2], case[3])[0]
    again = [k for k, v in res.items() if v[2] >= 1]
    assert len(again) >= 2, again
    if polarity == -1:
        assert [k for k, v in res.items() if -32768 in v[3]]


def test_lpc_conditions():
    fs, n = 44100, 20000
    names, pcm = hs.matrix(hs.bank(fs, n, 0))
    kw = dict(order=12, window="rectangular", pre_emphasis=1, hop_s=0.0, window_s=16384 / 44100)
    assert lr.frame_plan(fs, n, lr.opts(**kw))[0] == lr.MAX_WINDOW
    want = lr.analyse(pcm, fs, **kw)
    assert (want["n_frames"] == 1).all()
    i = names.index("alternating")
    assert want["r0"][i, 0] > 4e18 and want["status"][i, 0] == 0
    # ... exactly 2^30 * 65535^2: one 32-product block is 2^21 * 65535^2, just under 2^53
    assert want["r0"][i, 0] == float(2 ** 30 * 65535 ** 2) and 0.9999 * 2 ** 53 < 2 ** 21 * 65535 ** 2 < 2 ** 53
    for k in ("constant", "constant_min", "zeros"):
        assert want["status"][names.index(k), 0] == lr.SILENT, k
    assert not (want["status"] == lr.UNSTABLE).any()
