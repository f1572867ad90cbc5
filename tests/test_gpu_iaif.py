"""The IAIF analysis on the device (vs_iaif / vs_iaif_launch, bin/vinverse -I, bin/formants -I) against its numpy
restatement (tests/iaif_ref.py): r0, err, start, status, coefs (V2) and glottal (c2) bit for bit, compared as int64
views with NaN patterns by isnan; the formants within the header's VS_LPC_FORMANT_TOL_HZ of numpy.roots of the device's
own V2.  Shapes are the smallest that take the kernel's seams: two window lengths in one call, rows with 0 and 1 frame,
frame counts that are no multiple of the frames per workgroup, windows that are no multiple of the LDS chunk, frames
with less history than M before them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_signals as hs  # noqa: E402
import iaif_ref as ia  # noqa: E402
from test_gpu_lpc import _cli_line, _pipeline, _read, assert_formants  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
CHUNK = 64                       # VS_LPC_CHUNK of csrc/vs_lpc.h
N_MIXED, NS_MIXED = 48, 3000


def frames_per_workgroup(order):
    """vs_lpc_fb of csrc/vs_lpc.h"""
    return min(64, 256 // ((order + 1 + 3) // 4))


def same_bits(g, w):
    g, w = np.ascontiguousarray(g, np.float64), np.ascontiguousarray(w, np.float64)
    nan = np.isnan(g) & np.isnan(w)
    return nan | ((g.view(np.int64) == w.view(np.int64)) & ~np.isnan(g) & ~np.isnan(w))


def assert_exact(got, want, keys=("r0", "err", "coefs", "glottal")):
    assert np.array_equal(got["n_frames"], want["n_frames"])
    assert np.array_equal(got["start"], want["start"])
    # VS_LPC_NO_ROOTS is the root finder's verdict, outside the exact part (the restatement uses numpy.roots)
    st = np.where(got["status"] == vs.VS_LPC_NO_ROOTS, 0, got["status"])
    assert np.array_equal(st, want["status"]), np.argwhere(st != want["status"])[:8]
    for k in keys:
        same = same_bits(got[k], want[k])
        assert same.all(), (k, np.argwhere(~same)[:8])


_mixed = {}


def mixed_rows(engine):
    """48 rows of 3000 samples: the vowels of ten tables at 16000 and 22050 Hz in turn (L = 400 and 551, H = 160 and
    221), lengths 400..3000: row 2 has one frame (400 samples at 16 kHz), row 3 none (400 at 22050 Hz), row 5 none (0)"""
    if not _mixed:
        rows = np.zeros((N_MIXED, NS_MIXED), dtype=np.int16)
        fs = np.where(np.arange(N_MIXED) % 2 == 0, 16000, 22050).astype(np.int32)
        for rate in (16000, 22050):
            idx = np.flatnonzero(fs == rate)
            rate_arg = ["-r", str(rate)] if rate != 22050 else []
            lanes = [vs.lane_from_cli(rate_arg + ["-d", "1", "-f", str(90 + k), "-s", "5", "-j", "1"],
                                      ["-v", "aiu1234567"[k % 10]], 40 + k)[0] for k in range(len(idx))]
            rows[idx] = engine.synth(lanes, NS_MIXED)
        lengths = np.random.default_rng(7).integers(400, NS_MIXED + 1, N_MIXED).astype(np.int32)
        lengths[0] = lengths[1] = NS_MIXED
        lengths[2] = lengths[3] = 400
        lengths[5] = 0
        rows.setflags(write=False)
        _mixed.update(pcm=rows, fs=fs, lengths=lengths)
    return _mixed["pcm"], _mixed["fs"], _mixed["lengths"]


MIXED_CASES = {
    "p22-g4": dict(order=22, glottal_order=4),
    "p1-g1": dict(order=1, glottal_order=1, n_formants=1),
    "p12-g2-rect-leak0.5": dict(order=12, glottal_order=2, window="rectangular", leak=0.5, n_formants=7),
    "p40-g6-leak1": dict(order=40, glottal_order=6, leak=1.0, n_formants=20),
    "p40-g40-leak0": dict(order=40, glottal_order=40, leak=0.0, n_formants=3),
    "p22-g4-centre": dict(order=22, glottal_order=4, hop_s=0.0),
    "p12-g2-centre-rect": dict(order=12, glottal_order=2, hop_s=0.0, window="rectangular", leak=1.0),
}


@pytest.mark.parametrize("key", list(MIXED_CASES))
def test_mixed_rows_bit_for_bit(engine, key):
    pcm, fs, lengths = mixed_rows(engine)
    kw = MIXED_CASES[key]
    want = ia.analyse(pcm, fs, lengths, **kw)
    got = engine.iaif(pcm, fs, lengths=lengths, coefs=True, glottal=True, **kw)
    total, fb = int(got["n_frames"].sum()), frames_per_workgroup(kw["order"])
    assert got["n_frames"][5] == 0 and got["n_frames"][3] == 0
    if kw.get("hop_s", 0.01) > 0:
        assert got["n_frames"][2] == 1 and got["n_frames"][0] == 17 and got["n_frames"][1] == 12
        assert total % fb != 0 and total > 2 * fb             # more than one workgroup, the last one partly filled
        assert (np.cumsum(got["n_frames"]) % fb != 0).any()   # a row's frames straddle two workgroups
        assert got["start"][0, 0] == 0                        # history all zeros
    assert 400 % CHUNK != 0 and 551 % CHUNK != 0
    assert_exact(got, want)
    assert_formants(got, fs, kw.get("n_formants", 5))
    # without formants, coefficients and glottal sets: the same records
    bare = engine.iaif(pcm, fs, lengths=lengths, **dict(kw, n_formants=0))
    assert_exact(bare, want, keys=("r0", "err"))
    assert (bare["n_formants"][bare["status"] >= 0] == 0).all() and "coefs" not in bare and "glottal" not in bare


@pytest.mark.parametrize("order,g", [(22, 4), (40, 6)])
def test_frames_with_less_history_than_M(engine, order, g):
    """hop 1 ms: H = 16 and 22 samples, so the frames after the first start at 0 < s < M = order + 1, where the extended
    frame is part samples, part zeros; 38 and 21 frames per row straddle the workgroups of 42 and 23"""
    pcm, fs, _ = mixed_rows(engine)
    pcm, fs = pcm[:6, :1000], fs[:6]
    kw = dict(order=order, glottal_order=g, hop_s=0.001, n_formants=0)
    got = engine.iaif(pcm, fs, coefs=True, glottal=True, **kw)
    s = got["start"][0]
    assert s[0] == 0 and 0 < s[1] < order + 1 and got["n_frames"].sum() % frames_per_workgroup(order) != 0
    assert_exact(got, ia.analyse(pcm, fs, **kw))


@pytest.mark.parametrize("order,g", [(22, 4), (40, 6)])
def test_hostile_signals(engine, order, g):
    """noise, DC, tones, full scale, impulses (tests/hostile_signals.py): every status and every double of the exact
    part as the restatement has them; the formants' structure on every frame, and the header's tolerance on the noise
    rows, whose V2 is as well-conditioned as a vowel's"""
    fs, n, nmax = 16000, 4000, 5
    names, pcm = hs.matrix(hs.bank(fs, n, 0))
    kw = dict(order=order, glottal_order=g)
    want = ia.analyse(pcm, fs, **kw)
    got = engine.iaif(pcm, fs, coefs=True, glottal=True, **kw)
    assert_exact(got, want)
    for k in range(4):
        print("order %d status %d: %d frames" % (order, k, int((want["status"] == k).sum())))
    assert (got["status"][names.index("zeros")] == vs.VS_LPC_SILENT).all()
    dead = (want["status"] != 0) & (want["status"] >= 0)
    assert np.isnan(got["coefs"][dead][:, 1:]).all() and np.isnan(got["err"][dead]).all()
    assert np.isfinite(got["coefs"][want["status"] == 0]).all()
    for i in range(len(names)):
        for j in range(got["n_frames"][i]):
            st, nf, fm = got["status"][i, j], got["n_formants"][i, j], got["formants"][i, j]
            assert 0 <= nf <= nmax and np.isnan(fm[nf:]).all() and not np.isnan(fm[:nf]).any(), (names[i], j)
            assert st == 0 or nf == 0, (names[i], j)
            f = fm[:nf, 0]
            assert (np.diff(f) >= 0).all() and (f >= 50.0).all() and (f <= fs / 2 - 50.0).all(), (names[i], j, f)
    good = [names.index(k) for k in hs.NOISE_ROWS]
    assert (got["status"][good] == 0).all()
    assert_formants(got, fs, nmax, rows=good)


def test_a_larger_frames_pitch_and_what_no_frame_covers(engine):
    pcm, fs, lengths = mixed_rows(engine)
    pcm, fs, lengths = np.ascontiguousarray(pcm[:12]), fs[:12], lengths[:12]
    p, g, nfm = 22, 4, 5
    want = engine.iaif(pcm, fs, lengths=lengths, coefs=True, glottal=True)
    n, ns = pcm.shape
    fpitch = int(want["n_frames"].max()) + 3
    sizes = (n * fpitch * 32, n * fpitch * 2 * nfm * 8, n * fpitch * (p + 1) * 8, n * fpitch * (g + 1) * 8)
    with engine.scope() as dev:
        ptrs = [dev.room(b) for b in (pcm.nbytes,) + sizes]
        engine.dev_upload(ptrs[0], pcm)
        for ptr, b in zip(ptrs[1:], sizes):
            engine.dev_upload(ptr, np.full(b, 0x5A, dtype=np.uint8))
        engine.iaif_dev(ptrs[0], ns, n, ns, fs, fpitch, ptrs[1], ptrs[2], ptrs[3], ptrs[4], lengths=lengths)
        engine.synchronize()
        out = [engine.dev_download(ptr, (b,), np.uint8) for ptr, b in zip(ptrs[1:], sizes)]
    fr = out[0].view(vs.LPC_FRAME_DTYPE).reshape(n, fpitch)
    fm = out[1].view(np.float64).reshape(n, fpitch, nfm, 2)
    cf = out[2].view(np.float64).reshape(n, fpitch, p + 1)
    gl = out[3].view(np.float64).reshape(n, fpitch, g + 1)
    for i in range(n):
        nf = want["n_frames"][i]
        for k in ("r0", "err", "start", "status", "n_formants"):
            assert np.array_equal(fr[k][i, :nf], want[k][i, :nf], equal_nan=True), k
        assert (fr["reserved_"][i, :nf] == 0).all()
        assert same_bits(cf[i, :nf], want["coefs"][i, :nf]).all() and same_bits(gl[i, :nf], want["glottal"][i, :nf]).all()
        assert same_bits(fm[i, :nf], want["formants"][i, :nf]).all()
        assert (out[0].reshape(n, fpitch, 32)[i, nf:] == 0x5A).all()
        for a in (fm, cf, gl):
            assert (np.ascontiguousarray(a[i, nf:]).view(np.uint8) == 0x5A).all()


def test_the_chain_on_one_stream_equals_the_host_calls(engine):
    """iaif_dev -> inverse_filter_dev -> measure_dev without a host round trip, against iaif -> inverse_filter -> measure"""
    fs, n = 22050, 8
    lanes = [vs.lane_from_cli(["-d", "0.5", "-f", "100", "-s", "5"], ["-v", "a"], 300 + k)[0] for k in range(n)]
    ns = vs.num_samples(fs, 0.5)
    pcm = engine.synth(lanes, ns)
    p = 22
    lo = vs.iaif_lpc_opts(n_formants=0)
    nfr = vs.lpc_frames(fs, ns, **lo)
    row = vs.inverse_from_lpc(fs, ns, "hold", **lo)
    row["scale"], row["de_emphasis"] = 0.1, 0.99
    pitch = vs.row_pitch(ns)
    padded = np.zeros((n, pitch), dtype=np.int16)
    padded[:, :ns] = pcm
    sizes = (padded.nbytes, padded.nbytes, n * nfr * 32, n * nfr * (p + 1) * 8, n * vs.INVERSE_STAT_DTYPE.itemsize,
             n * vs.ACOUSTIC_DTYPE.itemsize)
    with engine.scope() as dev:
        pcm_d, flow_d, fr_d, cf_d, st_d, ac_d = ptrs = [dev.room(b) for b in sizes]
        engine.dev_upload(pcm_d, padded)
        engine.dev_upload(flow_d, np.zeros_like(padded))
        engine.iaif_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, None, cf_d, None, n_formants=0)
        engine.inverse_filter_dev("hold", p, pcm_d, pitch, flow_d, pitch, n, ns, row, cf_d, nfr, st_d)
        engine.measure_dev(flow_d, pitch, n, ns, fs, ac_d)
        engine.synchronize()
        flow = engine.dev_download(flow_d, (n, pitch))[:, :ns]
        stat = engine.dev_download(st_d, (n,), vs.INVERSE_STAT_DTYPE)
        ac = engine.dev_download(ac_d, (n,), vs.ACOUSTIC_DTYPE)
    sets = engine.iaif(pcm, fs, coefs=True, n_formants=0)
    assert (sets["status"] == 0).all()
    want_flow, want_stat = engine.inverse_filter(pcm, sets["coefs"], row["hop"], row["offset"], scale=0.1, de_emphasis=0.99)
    want_ac = engine.measure(want_flow, fs)
    assert np.array_equal(flow, want_flow) and np.array_equal(stat, want_stat)
    assert ac.tobytes() == want_ac.tobytes() and (ac["status"] == 0).all()


def test_bad_arguments_are_refused(engine):
    with engine.scope() as dev:
        pd = dev.room(2 * 4000 * 2)
        buf = dev.room(2 * 100 * 41 * 8 * 2)
        for kw in ({"glottal_order": 0}, {"glottal_order": 23}, {"order": 4, "glottal_order": 5}, {"leak": -0.1},
                   {"leak": 1.5}, {"leak": float("nan")}, {"order": 0}, {"order": 41}, {"window": 5}, {"n_formants": 21}):
            with pytest.raises(vs.VsError):
                engine.iaif_dev(pd, 4000, 2, 4000, 16000, 100, buf, **kw)
        with pytest.raises(vs.VsError):   # 23 frames > frames_pitch 22
            engine.iaif_dev(pd, 4000, 2, 4000, 16000, 22, buf)
        engine.synchronize()


# ---- the programs ----

def _run(tmp_path, prog, *args):
    return subprocess.run([os.path.join(BIN, prog)] + list(args), cwd=tmp_path, capture_output=True, text=True,
                          env=dict(os.environ, VS_WAV_HEADER="44"))


def test_programs_with_and_without_I(engine, tmp_path):
    f = _pipeline(tmp_path, "x", ["-r", "16000", "-d", "0.5", "-f", "110", "-s", "5"], ["-v", "a"], 21)
    x, fs = _read(tmp_path / f, 44)
    ns = len(x)
    # formants -I: the line of Engine.iaif; without -I: the line of Engine.lpc, as before
    for args, res in ((["-I"], engine.iaif(x[None], fs)),
                      (["-I", "-g", "6", "-l", "0.95", "-o", "18", "-n", "4"],
                       engine.iaif(x[None], fs, order=18, glottal_order=6, leak=0.95, n_formants=4)),
                      ([], engine.lpc(x[None], fs))):
        r = _run(tmp_path, "formants", *args, f)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == 2 and lines[1] == _cli_line(f, res, 0, res["formants"].shape[2]), args
    for args in (["-I", "-p", f], ["-g", "3", f], ["-l", "0.5", f], ["-I", "-g", "23", f], ["-I", "-l", "1.5", f]):
        assert _run(tmp_path, "formants", *args).returncode == 1, args
    # vinverse -I -m x.wav -i x.wav: the Python chain; without -I: the LPC residual, as before
    for extra, sets in ((["-I"], engine.iaif(x[None], fs, coefs=True, n_formants=0)),
                        (["-I", "-g", "6", "-l", "1", "-O", "18"],
                         engine.iaif(x[None], fs, coefs=True, n_formants=0, order=18, glottal_order=6, leak=1.0)),
                        ([], engine.lpc(x[None], fs, coefs=True, n_formants=0))):
        order = sets["coefs"].shape[2] - 1
        row = vs.inverse_from_lpc(fs, ns, "hold", order=order, n_formants=0)
        r = _run(tmp_path, "vinverse", "-i", f, "-o", "y.wav", "-m", f, "-s", "0.1", "-d", "0.99", *extra)
        assert r.returncode == 0, r.stderr
        want, st = engine.inverse_filter(x[None], sets["coefs"], row["hop"], row["offset"], scale=0.1, de_emphasis=0.99)
        assert r.stdout == "y.wav %d %d %d %d\n" % (row["n_sets"], st["n_unusable"][0], st["n_clipped"][0], st["status"][0])
        assert np.array_equal(_read(tmp_path / "y.wav", 44)[0], want[0]), extra
    base = ["-i", f, "-o", "z.wav"]
    for args in (base + ["-I", "-v", "a"], base + ["-I", "-P", "-m", f], base + ["-g", "4", "-m", f],
                 base + ["-l", "0.9", "-m", f], base + ["-I", "-g", "23", "-m", f], base + ["-I", "-l", "2", "-m", f]):
        assert _run(tmp_path, "vinverse", *args).returncode == 1, args
        assert not os.path.exists(tmp_path / "z.wav")
