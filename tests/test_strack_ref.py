"""The source track's restatement (tests/strack_ref.py) on the CPU: on a constant track it is the oracle's vs_oracle_source
sample for sample, cycle for cycle and draw for draw, whatever the frames look like; the corners of the walk; and the
closed loop pitch track -> source track -> pitch track -> guided marks, all from restatements.  And the library's
device-free half: the row that plays the pitch track's frames.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voice_synth_amd as vs  # noqa: E402
from oracle import pyoracle  # noqa: E402
import guided_ref as gr  # noqa: E402
import pitch_ref as pt  # noqa: E402
import pitch_signals as ps  # noqa: E402
import strack_ref as sr  # noqa: E402

NS = 6000
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def lane_of(args, seed=12345):
    return vs.lane_from_cli(list(args), ["-v", "a"], seed=seed)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. a constant track is pyoracle.source_one ----

@pytest.mark.parametrize("args", sr.CONSTANT_LANES, ids=lambda a: " ".join(a) or "plain")
def test_constant_track_is_the_oracles_source(args):
    lane = lane_of(args)
    P = sr.constant_period(lane)
    want, recs, ncyc, ndraws = pyoracle.source_one(lane, NS, 4000)
    # hop 1, a hop beyond the row, offsets far to either side, one frame: f(n) differs, the period it finds does not
    for n_frames, hop, offset in ((8, 1, 0), (3, NS + 1000, 0), (40, 160, 5000), (40, 160, -5000), (1, 160, 0),
                                  (5, INT32_MAX, INT32_MIN)):
        flow, stat, cyc = sr.source_track_one(lane, NS, sr.row(n_frames, hop, offset, NS), [P] * n_frames)
        what = (args, n_frames, hop, offset)
        assert np.array_equal(flow, want), what
        assert int(stat["n_cycles"]) == ncyc and int(stat["n_draws"]) == ndraws and int(stat["status"]) == 0, what
        assert int(stat["n_resets"]) == 0 and int(stat["n_unvoiced"]) == 0, what
        assert np.array_equal(cyc["T"], recs["T"]), what
        for k in ("S", "x_pow", "w_pow"):
            assert np.array_equal(bits(cyc[k]), bits(recs[k])), (what, k)
        assert np.array_equal(cyc["start"], np.concatenate([[0], np.cumsum(recs["T"])[:-1]])), what
        assert (cyc["amp"] == lane.amp).all()


# ---- 2. corners of the walk ----

PLAIN = ["-r", "16000"]


def test_rows_that_begin_end_or_stay_unvoiced():
    lane = lane_of(["-l", "0.1"] + PLAIN)
    dcs = sr.short_of(int(lane.DC))
    assert dcs == 1200    # -l is a fraction of the default amplitude, 12000
    r = sr.row(4, 500, 100, 2000, 32, 320)
    # begins unvoiced: frame 0 governs everything before offset + hop
    flow, stat, cyc = sr.source_track_one(lane, 2000, r, [0, 100, 100, 100])
    assert (flow[:600] == dcs).all() and int(cyc["start"][0]) == 600 and int(stat["n_unvoiced"]) == 600
    assert int(stat["n_draws"]) == int(stat["n_cycles"]) == len(cyc) == 14 and int(stat["status"]) == 0
    # ends unvoiced: the last cycle of the voiced stretch runs to its end, the rest is DC
    flow, stat, cyc = sr.source_track_one(lane, 2000, r, [100, 100, 0, 0])
    end = int(cyc["start"][-1] + cyc["T"][-1])
    assert end == 1100 and (flow[end:] == dcs).all() and int(stat["n_unvoiced"]) == 2000 - end
    # a hole: the state starts again behind it (the flow behind the hole is the flow of a row that starts there)
    flow, stat, cyc = sr.source_track_one(lane_of(["-j", "2", "-s", "5"] + PLAIN), 2000, r, [100, 5, 100, 100])
    assert (cyc["frame"] != 1).all() and int(stat["n_unvoiced"]) > 0
    # no voiced frame: all (short)DC, VS_ST_NO_VOICED, no draw
    flow, stat, cyc = sr.source_track_one(lane, 2000, r, [0, 31, 321, -7])
    assert (flow == dcs).all() and int(stat["status"]) == sr.ST_NO_VOICED and int(stat["n_draws"]) == 0
    assert int(stat["n_unvoiced"]) == 2000 and len(cyc) == 0


def test_length_zero_and_samples_past_length():
    lane = lane_of(PLAIN)
    out = np.full(500, 0x5A5A, dtype=np.int16)
    flow, stat, cyc = sr.source_track_one(lane, 500, sr.row(1, 10, 0, 0), [100], out=out)
    assert (flow == 0x5A5A).all() and int(stat["status"]) == sr.ST_NO_VOICED and int(stat["n_cycles"]) == 0
    flow, stat, cyc = sr.source_track_one(lane, 500, sr.row(1, 10, 0, 250), [100], out=out)
    assert (flow[250:] == 0x5A5A).all() and int(stat["n_cycles"]) == 3
    whole, _, _ = sr.source_track_one(lane, 500, sr.row(1, 10, 0, 500), [100])
    assert np.array_equal(flow[:250], whole[:250])


def test_periods_and_amplitudes_outside_their_ranges_are_unvoiced():
    lane = lane_of(["-s", "5"] + PLAIN)
    r = sr.row(8, 200, 0, 1600)
    per = [100, 0, -5, INT32_MIN, INT32_MAX, 1, 2049, 100]
    flow, stat, cyc = sr.source_track_one(lane, 1600, r, per)
    assert set(cyc["frame"].tolist()) == {0, 7} and int(stat["n_unvoiced"]) == 1200
    amp = [8000, -1, 32767, 32766, 0, INT32_MIN, INT32_MAX, 8000]
    flow, stat, cyc = sr.source_track_one(lane, 1600, r, [100] * 8, amp)
    assert set(cyc["frame"].tolist()) == {0, 3, 4, 7}
    assert (cyc["amp"][cyc["frame"] == 4] == 0).all() and (flow[800:1000] == 0).all()    # amplitude 0 is voiced, and silent
    with pytest.raises(ValueError):
        sr.source_track_one(lane, 1600, sr.row(8, 200, 0, 1600, 1, 320), per)
    with pytest.raises(ValueError):
        sr.source_track_one(lane, 1600, sr.row(9, 200, 0, 1600), per)


def test_an_octave_drop_is_followed_without_a_reset():
    """300 -> 20 -> 7 -> 300 at -j 0.05: the rescaled DeltaPer stays inside 0.2 P.  Four frames of 730 samples: 139
    cycles in 3200 samples."""
    lane = lane_of(["-j", "0.05"] + PLAIN, seed=7)
    flow, stat, cyc = sr.source_track_one(lane, 3200, sr.row(4, 730, 0, 3200), [300, 20, 7, 300])
    assert int(stat["n_resets"]) == 0 and int(stat["n_cycles"]) == 139 and int(stat["n_draws"]) == 278
    for f, P in enumerate((300, 20, 7, 300)):
        T = cyc["T"][cyc["frame"] == f]
        assert len(T) and (np.abs(T - P) <= 0.2 * P).all()


def test_max_reject_ends_a_rejection_loop():
    """-j 1000 (a jitter of 10) rejects nearly every draw: with max_reject 4, 36 of the 38 cycles of 6000 samples at
    P = 160 end their loop by the cap, take T = P, and keep the four draws they made"""
    lane = lane_of(["-j", "1000"] + PLAIN, seed=7)
    flow, stat, cyc = sr.source_track_one(lane, NS, sr.row(1, 100, 0, NS), [160], max_reject=4)
    assert int(stat["n_resets"]) == 36 and int(stat["n_cycles"]) == 38 and int(stat["n_draws"]) == 187
    assert (cyc["T"] == 160).sum() >= 36


# ---- 3. the closed loop, from the restatements ----

COPY = ["-c", "0.6", "-a", "8000", "-r", "16000"]


@pytest.fixture(scope="module")
def loops():
    out = {}
    for name, sig in (("glide", ps.glide()), ("gaps", ps.gaps())):
        x = np.asarray(sig[0] if isinstance(sig, tuple) else sig, dtype=np.int16)
        model = pt.track_row(x, 16000)
        r = sr.row_from_pitch(16000, len(x))
        flow, stat, cyc = sr.source_track_one(lane_of(COPY, seed=1), len(x), r, model["lag"])
        copy = pt.track_row(flow, 16000)
        out[name] = dict(model=model, copy=copy, stat=stat, cyc=cyc, row=r, guided=gr.guided_row(flow, 16000, copy))
    return out


def voiced(fr):
    return (fr["lag"] >= 32) & (fr["lag"] <= 320)


def test_the_copy_of_the_glide_has_the_models_track(loops):
    g = loops["glide"]
    assert len(g["model"]) == len(g["copy"]) == 82 and voiced(g["model"]).all() and voiced(g["copy"]).all()
    d = g["copy"]["lag"].astype(int) - g["model"]["lag"].astype(int)
    assert d.min() == 0 and d.max() == 2
    assert int(g["stat"]["n_cycles"]) == 100 and int(g["stat"]["n_unvoiced"]) == 0
    assert g["guided"]["guided"][0] == 1 and len(g["guided"]["marks"]) == 100


def test_the_copy_of_the_gaps_pauses_where_the_model_does(loops):
    g = loops["gaps"]
    assert int(g["stat"]["n_unvoiced"]) == 8615
    vm, vc = voiced(g["model"]), voiced(g["copy"])
    assert vm.sum() == 89 and vc.sum() == 92 and (vm & vc).sum() == 89
    d = (g["copy"]["lag"].astype(int) - g["model"]["lag"].astype(int))[vm & vc]
    assert d.min() == 0 and d.max() == 1
    assert g["guided"]["guided"][0] == 2


# ---- the library's device-free half ----

def test_strack_row_from_pitch_is_the_guided_marks_frame_of_a_sample():
    for fs, length, kw in ((16000, 14026, {}), (16000, 962, {}), (44100, 30000, dict(f0_min=60.0, hop_s=0.005)),
                           (8000, 5000, dict(f0_max=400.0))):
        r = vs.strack_row_from_pitch(fs, length, **kw)
        want = sr.row_from_pitch(fs, length, **kw)
        assert r.tobytes() == want.tobytes(), (fs, length, r, want)
        tmin, tmax, H, nf, C = gr.plan(fs, length, gr.opts(**kw))
        for n in list(range(0, length, 97)) + [C, C + 1, length - 1]:
            assert sr.frame_of(n, int(r["offset"]), int(r["hop"]), nf) == gr.frame_of(n, C, H, nf), (fs, n)
    with pytest.raises(vs.VsError) as e:
        vs.strack_row_from_pitch(16000, 961)
    assert e.value.code == vs._ffi.VS_ERR_RANGE
    o = vs.strack_opts()
    assert o.max_reject == 256 and o.reserved_ == 0
