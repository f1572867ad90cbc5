"""The pitch track as include/voice_synth.h defines it ("pitch track"), on its numpy restatement (tests/pitch_ref.py): the
Lg table against the library's, the constructed signals (a glide, pauses, an octave trap, a subharmonic), and the
first-pass residuals of the 16 oracle vowels on which vs_measure's one window takes an octave error.  No device."""
import os
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acoustic_ref as ar  # noqa: E402
import cplpc_ref as cp  # noqa: E402
import pitch_ref as pr  # noqa: E402
import pitch_signals as ps  # noqa: E402

FS = 16000


def cands_of(r):
    return list(zip(r["cand_lag"][:r["n_cand"]].tolist(), r["cand_q"][:r["n_cand"]].tolist()))


def test_the_log2_table_is_the_librarys_and_far_from_a_tie():
    want = pr.log2_table()
    assert np.array_equal(vs.pitch_log2_table(), want) and want[1] == 0 and want[2] == 256 and want[2048] == 2816
    assert np.array_equal(vs.pitch_log2_table(17), want[:17])
    margin = pr.log2_margin()
    print("smallest distance of 256*log2(t) to a rounding tie, t <= 2048: %.2e" % margin)
    assert margin > 1e-6


def test_frames_and_refusals_agree_with_the_library():
    for fs, ln in ((16000, 0), (16000, 961), (16000, 962), (16000, 962 + 159), (16000, 962 + 160), (8000, 4000),
                   (22050, 22050), (44100, 3000), (96000, 96000)):
        tmin, tmax = ar.lag_bounds(fs)
        assert vs.pitch_frames(fs, ln) == pr.frame_count(ln, tmax, pr.hop(fs, 0.010)), (fs, ln)
    assert vs.pitch_frames(16000, 16000, hop_s=0.001) == 940
    for bad in (dict(voicing_q=-1), dict(octave_q=(1 << 20) + 1), dict(jump_q=-5), dict(vuv_q=1 << 21),
                dict(silence_rms=-1), dict(silence_rms=32768), dict(hop_s=float("nan")), dict(hop_s=-0.01), dict(f0_min=0.0)):
        with pytest.raises(vs.VsError) as e:
            vs.pitch_frames(16000, 16000, **bad)
        assert e.value.code == vs._ffi.VS_ERR_ARG, bad
    for bad in (dict(hop_s=0.0), dict(hop_s=1e-6), dict(f0_min=7.0), dict(f0_max=9000.0), dict(hop_s=1e9)):
        with pytest.raises(vs.VsError) as e:
            vs.pitch_frames(16000, 16000, **bad)
        assert e.value.code == vs._ffi.VS_ERR_RANGE, bad
    assert vs.pitch_frames(16000, 16000, voicing_q=0, octave_q=1 << 20, silence_rms=0) == 94


def test_a_glide_is_followed():
    """periods from 220 down to 80 at 16 kHz: every frame voiced, the path's lag within [-1, +2] of the period of the
    cycle under the frame's centre -- where vs_measure's one window gives one P0 for the whole row"""
    x, peaks, periods = ps.glide()
    rec = pr.track_row(x, FS)
    tmin, tmax = ar.lag_bounds(FS)
    starts = np.cumsum([0] + periods)
    d = []
    for r in rec:
        k = int(np.searchsorted(starts, int(r["start"]) + (3 * tmax) // 2, side="right")) - 1
        d.append(int(r["lag"]) - periods[min(k, len(periods) - 1)])
    print("glide: %d frames, lag - period in [%d, %d]" % (len(rec), min(d), max(d)))
    assert len(rec) > 60 and (rec["lag"] > 0).all() and (rec["status"] == 0).all()
    assert min(d) >= -1 and max(d) <= 2
    assert rec["lag"][0] > 200 and rec["lag"][-1] < 100


def test_voicing_is_decided():
    """a train, 4000 zeros, 5000 samples of noise, the train again: voiced over the trains, unvoiced between them (the
    zeros silent, the noise with candidates the path does not take)"""
    x = ps.gaps()
    rec = pr.track_row(x, FS)
    tmin, tmax = ar.lag_bounds(FS)
    centre = rec["start"] + (3 * tmax) // 2
    voiced = rec["lag"] > 0
    n1 = 60 * 123
    assert voiced[centre < n1 - tmax].all() and voiced[centre > n1 + 9000 + tmax].all()
    between = (centre > n1 + tmax) & (centre < n1 + 9000 - tmax)
    assert between.sum() > 40 and not voiced[between].any()
    assert ((rec["status"][between] & pr.PT_UNVOICED) != 0).all()
    assert set(rec["lag"][voiced].tolist()) <= {122, 123, 124}
    assert int(np.count_nonzero(voiced[1:] & ~voiced[:-1])) + int(voiced[0]) == 2          # two segments
    zeros = (rec["start"] >= n1) & (rec["start"] + 3 * tmax < n1 + 4000)
    assert zeros.any() and (rec["status"][zeros] == (pr.PT_SILENT | pr.PT_UNVOICED)).all() and (rec["r0"][zeros] == 0).all()
    noise = (rec["start"] >= n1 + 4000) & (rec["start"] + 3 * tmax < n1 + 9000)
    best = [max(q for _, q in cands_of(r)) for r in rec[noise]]
    print("best q in the noise: %d .. %d of 32768" % (min(best), max(best)))
    assert noise.any() and max(best) < 14746 - 4588


def test_the_path_differs_from_the_greedy_pick():
    x = ps.octave_trap()
    rec = pr.track_row(x, FS)
    greedy = [pr.greedy(cands_of(r)) for r in rec]
    print("octave trap: greedy picks 80 in %d of %d frames" % (greedy.count(80), len(rec)))
    assert (rec["lag"] == 160).all()
    assert greedy.count(80) >= 1


def test_the_octave_cost_decides_a_subharmonic():
    x = ps.subharmonic()
    assert set(pr.track_row(x, FS)["lag"].tolist()) == {200}
    assert set(pr.track_row(x, FS, octave_q=3277)["lag"].tolist()) == {100}


def test_ties_of_a_square_go_to_the_smaller_lag():
    """a full-scale square of period 40 ties q at 40, 80, 120 ...: candidates in ascending lag, the path on the first"""
    x = np.where((np.arange(4000) // 20) % 2 == 0, 32767, -32767).astype(np.int16)
    rec = pr.track_row(x, 8000)
    assert (rec["n_cand"] >= 2).all()
    for r in rec:
        c = cands_of(r)
        assert [t for t, _ in c] == sorted(t for t, _ in c) and c[0][0] == 40 and len({q for _, q in c}) == 1
    assert (rec["lag"] == 40).all() and (rec["q"] == 32768).all()


def oracle_rows(args):
    from oracle import pyoracle
    specs = [(["-d", "1", "-f", "100"] + list(args), ["-v", "a"], 300 + k) for k in range(16)]
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(22050, d)
    pcm = pyoracle.synth(lanes, ns)
    return pcm, cp.first_pass(pcm, 22050, scale=1.0 / lanes[0].gain, first_de_emphasis=1.0)


def test_the_octave_row_of_the_oracle_vowels_is_repaired():
    """-s 10 at f0_min 50: vs_measure's restatement marks row 6 at period 440 for 220; the path stays within [215, 225]
    in every frame of all 16 rows"""
    pcm, first = oracle_rows(("-s", "10"))
    assert first["meas"]["p0"].tolist() == [220] * 6 + [440] + [220] * 9
    rec, nfr = pr.track(first["residual"], 22050)
    n440 = []
    for i in range(16):
        r = rec[i, :nfr[i]]
        assert nfr[i] > 80 and ((r["lag"] >= 215) & (r["lag"] <= 225)).all(), (i, sorted(set(r["lag"].tolist())))
        n440.append([pr.greedy(cands_of(f)) for f in r].count(440))
    print("frames whose greedy pick is 440, per row:", n440)
    assert sum(n440) > 0            # the transition costs do that work, not the candidates


def test_where_it_does_worse():
    """printed, not hidden: flowgen -n 20 (noise in the source) and a row shorter than one frame"""
    pcm, first = oracle_rows(("-s", "2", "-n", "20"))
    rec, nfr = pr.track(first["residual"], 22050)
    out = sum(int(((rec[i, :nfr[i]]["lag"] < 215) | (rec[i, :nfr[i]]["lag"] > 225)).sum()) for i in range(16))
    unv = sum(int((rec[i, :nfr[i]]["lag"] == 0).sum()) for i in range(16))
    print("-s 2 -n 20: %d of %d frames outside [215, 225], %d of them unvoiced" % (out, int(nfr.sum()), unv))
    short = pr.track_row(np.zeros(961, np.int16), FS)
    assert len(short) == 0
