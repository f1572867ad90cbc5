"""The LPC analysis on the device (vs_lpc / vs_lpc_launch, bin/formants) against its numpy restatement
(tests/lpc_ref.py): r0, err, start, status and the coefficients bit for bit; the formants within the header's
VS_LPC_FORMANT_TOL_HZ of numpy.roots of the device's own A, with equal counts; and against the truth of the ten tables."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import voice_synth_amd as vs
from voice_synth_amd import configs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_signals as hs  # noqa: E402
import lpc_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(vs.__file__), "bin")
TABLES = "aiu1234567"


def assert_exact(got, want, rows=None):
    rows = np.arange(got["r0"].shape[0]) if rows is None else rows
    assert np.array_equal(got["n_frames"][rows], want["n_frames"])
    assert np.array_equal(got["start"][rows], want["start"])
    # VS_LPC_NO_ROOTS is the root finder's verdict, outside the exact part (the restatement uses numpy.roots)
    st = np.where(got["status"][rows] == vs.VS_LPC_NO_ROOTS, 0, got["status"][rows])
    assert np.array_equal(st, want["status"]), np.argwhere(st != want["status"])[:8]
    for k in ("r0", "err", "coefs"):
        g, w = got[k][rows], want[k]
        same = (g == w) | (np.isnan(g) & np.isnan(w))
        assert same.all(), (k, np.argwhere(~same)[:8])


def assert_formants(got, fs, n_formants, f_lo=50.0, step=1, rows=None):
    """device formants against numpy.roots of the device's A on every step-th frame; the largest difference in Hz"""
    rows = np.arange(got["r0"].shape[0]) if rows is None else rows
    fs = np.broadcast_to(np.asarray(fs), (got["r0"].shape[0],))
    worst, k = 0.0, 0
    for i in rows:
        for j in range(got["n_frames"][i]):
            k += 1
            if k % step or got["status"][i, j] != 0:
                continue
            want = lr.formants_of(got["coefs"][i, j], int(fs[i]), n_formants, f_lo)
            nf = got["n_formants"][i, j]
            assert nf == len(want), (i, j, nf, want)
            g = got["formants"][i, j]
            assert np.isnan(g[nf:]).all()
            if nf:
                worst = max(worst, float(np.abs(g[:nf] - np.array(want)).max()))
    assert worst <= vs.VS_LPC_FORMANT_TOL_HZ, worst
    return worst


def _config_pcm(engine, index, n=None):
    specs, fs, dur, _ = configs.config_specs(index, n)
    lanes, d = vs.lanes_from_specs(specs)
    return engine.synth(lanes, vs.num_samples(fs, d)), fs


def test_parity_on_config2_in_full(engine):
    pcm, fs = _config_pcm(engine, 2)
    got = engine.lpc(pcm, fs, coefs=True)
    assert got["r0"].shape == (1024, 98) and (got["status"] == 0).all()
    assert_exact(got, lr.analyse(pcm, fs))
    assert_formants(got, fs, 5, step=7)


@pytest.mark.parametrize("index", [3, 5])
def test_parity_on_full_batches_compared_on_spread_rows(engine, index):
    pcm, fs = _config_pcm(engine, index)
    got = engine.lpc(pcm, fs, coefs=True)
    assert got["r0"].shape == (65536, 98)
    rows = np.linspace(0, 65535, 256).astype(int)
    assert_exact(got, lr.analyse(pcm[rows], fs), rows)
    assert_formants(got, fs, 5, step=5, rows=rows)
    assert (got["status"] == 0).mean() > 0.99


@pytest.mark.parametrize("order", [1, 12, 22, 40])
def test_parity_over_orders_windows_pre_emphasis_and_hops(engine, order):
    pcm, fs = _config_pcm(engine, 5, 96)
    for window in ("hamming", "rectangular"):
        for pre in (0, 1):
            for hop in (0.010, 0.0):
                kw = dict(order=order, window=window, pre_emphasis=pre, hop_s=hop, n_formants=min(20, order // 2 + 1))
                got = engine.lpc(pcm, fs, coefs=True, **kw)
                assert_exact(got, lr.analyse(pcm, fs, **kw))
                assert_formants(got, fs, kw["n_formants"], step=3 if hop else 1)


def _impulse_lanes(fs, vowels=TABLES):
    lanes = []
    for k, v in enumerate(vowels):
        lane = vs.lane_from_cli((["-r", str(fs)] if fs != 22050 else []) + ["-d", "1"], ["-v", v, "-p", "0", "-g", "1"],
                                k + 1)[0]
        lanes.append(lane)
    return lanes


def _impulse_responses(engine, lanes, n=4096):
    """filter a unit impulse, then one scaled to a peak of about 30000 (the filter is linear)"""
    flow = np.zeros((len(lanes), n), dtype=np.int16)
    flow[:, 0] = 100
    peak = np.abs(engine.filter(lanes, flow).astype(np.int64)).max(axis=1)
    flow[:, 0] = np.minimum(32767, 100 * 30000 // np.maximum(peak, 1))
    out = engine.filter(lanes, flow)
    assert np.abs(out).max() < 32767
    return out


def _centre_opts(fs, n=4096):
    return dict(order=22, window="rectangular", window_s=n / fs, hop_s=0, n_formants=20)


@pytest.mark.parametrize("fs", [16000, 22050, 44100])
def test_table_truth_on_the_device(engine, fs):
    lanes = _impulse_lanes(fs)
    h = _impulse_responses(engine, lanes)
    got = engine.lpc(h, fs, coefs=True, **_centre_opts(fs))
    assert (got["n_frames"] == 1).all() and (got["start"][:, 0] == 0).all() and (got["status"][:, 0] == 0).all()
    for k, v in enumerate(TABLES):
        want = lr.table_formants(vs.vowel_coefficients(v), fs)
        nf = got["n_formants"][k, 0]
        assert nf == len(want), (v, nf, len(want))
        assert np.abs(got["formants"][k, 0, :nf] - np.array(want)).max() <= 2.0 * fs / 16000, v


def test_copy_synthesis_round_trip(engine):
    """the recovered A, synthesised again through vs.set_coefficients and analysed again: the same formants within 1 Hz
    (measured 0.78 Hz: both impulse responses are rounded to int16, as in the table truth)"""
    fs = 16000
    lanes = _impulse_lanes(fs)
    first = engine.lpc(_impulse_responses(engine, lanes), fs, coefs=True, **_centre_opts(fs))
    copies = [vs.set_coefficients(lane, first["coefs"][k, 0]) for k, lane in enumerate(_impulse_lanes(fs))]
    again = engine.lpc(_impulse_responses(engine, copies), fs, coefs=True, **_centre_opts(fs))
    assert np.array_equal(again["n_formants"], first["n_formants"])
    for k in range(len(TABLES)):
        nf = first["n_formants"][k, 0]
        assert np.abs(again["formants"][k, 0, :nf] - first["formants"][k, 0, :nf]).max() <= 1.0, TABLES[k]


def test_device_chained_analysis_equals_the_host_path(engine):
    n = 4096
    specs, fs, dur, _ = configs.config_specs(3, n)
    lanes, d = vs.lanes_from_specs(specs)
    ns = vs.num_samples(fs, d)
    pitch = vs.row_pitch(ns)
    nfr = vs.lpc_frames(fs, ns)
    with engine.scope() as dev:
        plan = dev.plan(lanes, ns)
        pcm_d = dev.room(n * pitch * 2)
        fr_d = dev.room(n * nfr * 32)
        fm_d = dev.room(n * nfr * 10 * 8)
        cf_d = dev.room(n * nfr * 23 * 8)
        plan.launch(vs.VS_KIND_SYNTH, pcm_d, pitch)
        engine.lpc_dev(pcm_d, pitch, n, ns, fs, nfr, fr_d, fm_d, cf_d)
        assert plan.status() == 0
        fr = engine.dev_download(fr_d, (n, nfr), vs.LPC_FRAME_DTYPE)
        fm = engine.dev_download(fm_d, (n, nfr, 5, 2), np.float64)
        cf = engine.dev_download(cf_d, (n, nfr, 23), np.float64)
        pcm = engine.dev_download(pcm_d, (n, pitch))[:, :ns]
    want = engine.lpc(pcm, fs, coefs=True)
    for k in ("r0", "err", "start", "status", "n_formants"):
        assert np.array_equal(fr[k], want[k], equal_nan=k in ("r0", "err")), k
    assert np.array_equal(fm, want["formants"], equal_nan=True)
    assert np.array_equal(cf, want["coefs"], equal_nan=True)


def _sentinel_run(engine, pcm, fs, lengths, fpitch, n_formants=5, order=22, **kw):
    n, ns = pcm.shape
    fr_b, fm_b, cf_b = n * fpitch * 32, n * fpitch * max(1, 2 * n_formants) * 8, n * fpitch * (order + 1) * 8
    with engine.scope() as dev:
        pcm_d, fr_d, fm_d, cf_d = (dev.room(b) for b in (pcm.nbytes, fr_b, fm_b, cf_b))
        sent = [np.full(b, 0x5A, dtype=np.uint8) for b in (fr_b, fm_b, cf_b)]
        engine.dev_upload(pcm_d, pcm)
        for p, s in zip((fr_d, fm_d, cf_d), sent):
            engine.dev_upload(p, s)
        engine.lpc_dev(pcm_d, ns, n, ns, fs, fpitch, fr_d, fm_d, cf_d, lengths=lengths, n_formants=n_formants,
                       order=order, **kw)
        engine.synchronize()
        out = [engine.dev_download(p, (b,), np.uint8) for p, b in zip((fr_d, fm_d, cf_d), (fr_b, fm_b, cf_b))]
    return out, sent


def test_ragged_rows_mixed_rates_and_untouched_records(engine):
    rates = [16000, 22050, 44100]
    rows, fs, lengths = [], [], []
    rng = np.random.default_rng(3)
    for k in range(12):
        r = rates[k % 3]
        lane = _impulse_lanes(r, TABLES[k % 10])[0]
        flow = np.zeros((1, 24000), dtype=np.int16)
        flow[0, ::int(r / 110)] = 3000
        rows.append(engine.filter([lane], flow)[0])
        fs.append(r)
        lengths.append(int(rng.integers(8000, 24000)))
    lengths[4] = 100          # shorter than one 25 ms window at any of the rates
    lengths[8] = 1102         # one sample short of L = 1103 at 44.1 kHz
    pcm = np.array(rows)
    got = engine.lpc(pcm, fs, lengths=lengths, coefs=True)
    assert got["n_frames"][4] == 0 and got["n_frames"][8] == 0
    assert_exact(got, lr.analyse(pcm, fs, lengths=lengths))
    assert_formants(got, fs, 5)
    for i in range(12):
        alone = engine.lpc(pcm[i:i + 1, :lengths[i]], fs[i], coefs=True)
        nf = got["n_frames"][i]
        assert np.array_equal(alone["coefs"][0, :nf], got["coefs"][i, :nf], equal_nan=True)
    # what no frame covers stays as it was, in all three buffers
    fpitch = int(got["n_frames"].max()) + 3
    out, sent = _sentinel_run(engine, pcm, np.array(fs), np.array(lengths), fpitch)
    fr = out[0].view(vs.LPC_FRAME_DTYPE).reshape(12, fpitch)
    fm = out[1].view(np.float64).reshape(12, fpitch, 10)
    cf = out[2].view(np.float64).reshape(12, fpitch, 23)
    s8 = np.full(8, 0x5A, dtype=np.uint8).view(np.float64)[0]
    for i in range(12):
        nf = got["n_frames"][i]
        assert np.array_equal(fr[i, :nf]["r0"], got["r0"][i, :nf])
        assert (out[0].reshape(12, fpitch, 32)[i, nf:] == 0x5A).all()
        assert (fm[i, nf:].view(np.uint64) == s8.view(np.uint64)).all()
        assert (cf[i, nf:].view(np.uint64) == s8.view(np.uint64)).all()
        assert np.array_equal(cf[i, :nf], got["coefs"][i, :nf], equal_nan=True)


def test_silent_rows(engine):
    pcm = np.zeros((3, 4000), dtype=np.int16)
    pcm[1, 2000] = 5          # one non-zero sample: not silent in the two frames that hold it
    got = engine.lpc(pcm, 16000, coefs=True)
    # ... where A(z) = z^22, a 22-fold root at 0 that the root finder reports as VS_LPC_NO_ROOTS, taps and err valid
    assert (got["status"][1, 11:13] == vs.VS_LPC_NO_ROOTS).all() and (got["coefs"][1, 11:13, 1:] == 0).all()
    assert (got["err"][1, 11:13] == got["r0"][1, 11:13]).all() and (got["n_formants"][1] == 0).all()
    st = got["status"]
    assert (st[0] == vs.VS_LPC_SILENT).all() and (st[2] == vs.VS_LPC_SILENT).all()
    assert np.isnan(got["err"][0]).all() and np.isnan(got["coefs"][0, :, 1:]).all()
    assert (got["coefs"][0, :, 0] == 1.0).all() and (got["r0"][0] == 0).all()
    assert np.isnan(got["formants"][0]).all() and (got["n_formants"][0] == 0).all()
    assert_exact(got, lr.analyse(pcm, 16000))


# ---- signals the project does not synthesise (tests/hostile_signals.py) ----

_CENTRE = dict(window="rectangular", pre_emphasis=1, hop_s=0.0, window_s=16384 / 44100)   # L = VS_LPC_MAX_WINDOW
HOSTILE_CALLS = {"16k-o22-hamming": (16000, 8000, dict(order=22, window="hamming")),
                 "16k-o40-rect-pre": (16000, 8000, dict(order=40, window="rectangular", pre_emphasis=1)),
                 "44k-o22-hamming": (44100, 20000, dict(order=22, window="hamming")),
                 "44k-o40-rect-pre": (44100, 20000, dict(order=40, window="rectangular", pre_emphasis=1)),
                 "44k-o12-L16384": (44100, 20000, dict(order=12, **_CENTRE)),
                 "44k-o40-L16384": (44100, 20000, dict(order=40, **_CENTRE))}
_hostile_cache = {}


def _hostile(engine, key):
    """(names, pcm, fs, options, the device's answer with five formants and the coefficients) of one call, run once"""
    if key not in _hostile_cache:
        fs, n, kw = HOSTILE_CALLS[key]
        names, pcm = hs.matrix(hs.bank(fs, n, 0))
        _hostile_cache[key] = (names, pcm, fs, kw, engine.lpc(pcm, fs, coefs=True, n_formants=5, **kw))
    return _hostile_cache[key]


@pytest.mark.parametrize("key", list(HOSTILE_CALLS))
def test_hostile_signals_exact_part(engine, key):
    """noise, DC, full-scale squares, pure tones (reflection coefficients next to +-1), and the longest window: with
    pre-emphasis and a rectangular window of 16384 samples the alternating row has r0 = 2^30 * 65535^2 = 4.6e18, half of
    int64's range, out of 32-product blocks of 2^21 * 65535^2, 1.4e11 below 2^53"""
    names, pcm, fs, kw, got = _hostile(engine, key)
    want = lr.analyse(pcm, fs, **kw)
    assert_exact(got, want)
    assert not (want["status"] == lr.UNSTABLE).any()
    for k in ("constant", "constant_min", "zeros"):
        silent = (got["status"][names.index(k)] == vs.VS_LPC_SILENT).all()
        assert silent == bool(kw.get("pre_emphasis") or k == "zeros"), k
    if "L16384" in key:
        i = names.index("alternating")
        assert (got["n_frames"] == 1).all() and got["start"][i, 0] == 1 + (20000 - 1 - 16384) // 2
        assert got["r0"][i, 0] == want["r0"][i, 0] == float(2 ** 30 * 65535 ** 2) and got["r0"][i, 0] > 4e18
        assert got["status"][i, 0] & ~vs.VS_LPC_NO_ROOTS == 0


def _numpy_roots_and_their_newton_step(A, fs):
    """the roots of A by numpy.roots with Im z > 0, and how far one Newton step against the same A moves each of them,
    in Hz (the larger of |df| and |dbw|): what numpy.roots itself resolves of this A"""
    A = np.asarray(A, dtype=np.float64)
    z = np.roots(A)
    z = z[z.imag > 0]
    z1 = z - np.polyval(A, z) / np.polyval(np.polyder(A), z)

    def hz(v):
        return fs * np.arctan2(v.imag, v.real) / (2 * np.pi), -fs * np.log(np.abs(v)) / np.pi
    (f, bw), (f1, bw1) = hz(z), hz(z1)
    return np.maximum(np.abs(f1 - f), np.abs(bw1 - bw))


def hostile_formant_distances(names, fs, got, n_formants=5, f_lo=50.0):
    """per row: (frames with status 0, frames with VS_LPC_NO_ROOTS, of those the frames whose A(z) is z^p exactly, frames
    whose count differs from numpy.roots', worst |df| or |dbw| of the device against numpy.roots of its own A in Hz,
    worst Newton step of a numpy.roots root in Hz)"""
    table = {}
    for i, name in enumerate(names):
        ok = noroots = zp = miscount = 0
        worst = yard = 0.0
        for j in range(got["n_frames"][i]):
            st, A = got["status"][i, j], got["coefs"][i, j]
            if st == vs.VS_LPC_NO_ROOTS:
                noroots += 1
                zp += int((A[1:] == 0).all())
            if st != 0:
                continue
            ok += 1
            want = lr.formants_of(A, fs, n_formants, f_lo)
            nf = got["n_formants"][i, j]
            if nf != len(want):
                miscount += 1
                continue
            if nf:
                worst = max(worst, float(np.abs(got["formants"][i, j, :nf] - np.array(want)).max()))
            yard = max(yard, float(_numpy_roots_and_their_newton_step(A, fs).max(initial=0.0)))
        table[name] = (ok, noroots, zp, miscount, worst, yard)
    return table


@pytest.mark.parametrize("key", list(HOSTILE_CALLS))
def test_formants_on_hostile_signals(engine, key):
    """Structure on every frame; the header's VS_LPC_FORMANT_TOL_HZ against numpy.roots of the device's A on the noise rows
    and the sine in noise, whose A(z) is as well-conditioned as a vowel's.  On the other rows numpy.roots is not a fixed
    yardstick, so it is asked what it resolves itself: one Newton step against the same A moves its roots by some Hz, and
    the device is held, row by row, to 10 x the larger of that and the tolerance (10: from one root's correction to the
    pairing of two sets of roots).  VS_LPC_NO_ROOTS may appear on the constant and pure-tone rows, and on frames whose
    A(z) is z^p exactly, the p-fold root at 0 the header names (single-sample pulses further apart than the order).

    Measured on one MI355X (profiles/lpc_hostile_signals.txt): every count equals numpy.roots'; NO_ROOTS only on frames
    with A(z) = z^p (impulse and pulse trains at order 22, the first difference of the square wave), none on constants,
    tones or noise; every row but one within 2e-9 Hz (numpy's own step: up to 4e-9 Hz).  The impulse train at order 40
    with pre-emphasis is 3.0e-5 Hz (16 kHz) and 8.3e-5 Hz (44.1 kHz) from numpy.roots, whose roots move 1.5e-4 and
    4.1e-4 Hz under their Newton step: numpy's error, not the device's."""
    names, pcm, fs, kw, got = _hostile(engine, key)
    f_lo, nmax = 50.0, 5
    silent = lr.analyse(pcm, fs, **kw)["status"] == lr.SILENT
    for i in range(len(names)):
        for j in range(got["n_frames"][i]):
            st, nf, fm = got["status"][i, j], got["n_formants"][i, j], got["formants"][i, j]
            assert st in (0, vs.VS_LPC_NO_ROOTS) or (st == vs.VS_LPC_SILENT and silent[i, j]), (names[i], j, st)
            assert 0 <= nf <= nmax and np.isnan(fm[nf:]).all() and not np.isnan(fm[:nf]).any(), (names[i], j)
            assert st == 0 or nf == 0, (names[i], j)
            f = fm[:nf, 0]
            assert (np.diff(f) >= 0).all() and (f >= f_lo).all() and (f <= fs / 2 - f_lo).all(), (names[i], j, f)
    good = [names.index(k) for k in hs.NOISE_ROWS]
    assert (got["status"][good] == 0).all()
    assert_formants(got, fs, nmax, f_lo, rows=good)
    table = hostile_formant_distances(names, fs, got, nmax, f_lo)
    for name, (ok, noroots, zp, miscount, worst, yard) in table.items():
        print("%-18s %-15s frames %3d no_roots %3d (z^p %3d) miscount %d worst %.3e Hz numpy-newton %.3e Hz"
              % (key, name, ok, noroots, zp, miscount, worst, yard))
    for name, (ok, noroots, zp, miscount, worst, yard) in table.items():
        assert noroots == zp or name in hs.CROWDED_ROWS, (name, noroots, zp)
        assert miscount == 0, name
        assert worst <= 10.0 * max(yard, vs.VS_LPC_FORMANT_TOL_HZ), (name, worst, yard)


def test_no_formants_leaves_the_formant_buffer_untouched(engine):
    pcm, fs = _config_pcm(engine, 2, 8)
    out, sent = _sentinel_run(engine, pcm, fs, None, 98, n_formants=0)
    assert np.array_equal(out[1], sent[1])
    fr = out[0].view(vs.LPC_FRAME_DTYPE)
    assert (fr["n_formants"] == 0).all() and (fr["status"] == 0).all()


def test_bad_arguments_are_refused(engine):
    pcm = np.zeros((2, 4000), dtype=np.int16)
    with engine.scope() as dev:
        buf = dev.room(2 * 100 * 41 * 8 * 2)
        pd = dev.room(pcm.nbytes)
        for kw in ({"order": 0}, {"order": 41}, {"window_s": 1.2}, {"window_s": 0.001, "order": 22}, {"hop_s": 1e-6},
                   {"n_formants": 21}, {"window": 5}, {"pre_emphasis": 3}, {"f_lo": -1.0}):
            with pytest.raises(vs.VsError):
                engine.lpc_dev(pd, 4000, 2, 4000, 16000, 100, buf, **kw)
        with pytest.raises(vs.VsError):   # 23 frames > frames_pitch 22
            engine.lpc_dev(pd, 4000, 2, 4000, 16000, 22, buf)
        with pytest.raises(vs.VsError):   # a row longer than n_samples
            engine.lpc_dev(pd, 4000, 2, 4000, 16000, 100, buf, lengths=[4000, 4001])
        lib, fsa = vs.load(), np.full(2, 16000, dtype=np.int32)
        o = vs.lpc_opts()
        assert lib.vs_lpc_launch(engine._ctx, C.byref(o), C.c_void_p(pd), 4000, 2, 4000, fsa.ctypes.data, None, 100,
                                 None, None, None) == vs._ffi.VS_ERR_ARG
        o.reserved_ = 1
        assert lib.vs_lpc_launch(engine._ctx, C.byref(o), C.c_void_p(pd), 4000, 2, 4000, fsa.ctypes.data, None, 100,
                                 C.c_void_p(buf), None, None) == vs._ffi.VS_ERR_ARG
        engine.synchronize()


# ---- bin/formants ----

def _wav(path, fs, payload, header=44):
    data = payload.tobytes()
    if header == 44:
        h = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 1, fs, fs * 2, 2, 16,
                        b"data", len(data))
    else:
        buf = (C.c_ubyte * 72)()
        assert vs.load().vs_wav_header_write(buf, 72, fs, len(data) / 2.0 / fs) == 72
        h = bytes(buf)
    open(path, "wb").write(h + data)


def _pipeline(tmp_path, name, fa, va, seed, header=44):
    env = dict(os.environ, VS_SEED=str(seed), VS_WAV_HEADER=str(header))
    g = name + "_g.wav"
    subprocess.run([os.path.join(BIN, "flowgen_shimmer"), "-o", g] + fa, cwd=tmp_path, env=env, check=True,
                   capture_output=True)
    subprocess.run([os.path.join(BIN, "vowel"), "-i", g, "-o", name + ".wav"] + va, cwd=tmp_path, env=env, check=True,
                   capture_output=True)
    return name + ".wav"


def _read(path, header):
    raw = open(path, "rb").read()
    return np.frombuffer(raw[header:], dtype=np.int16), struct.unpack("<I", raw[24:28])[0]


def _fmt(v):
    return "nan" if np.isnan(v) else "%.3f" % v


def _cli_line(name, res, i, n):
    nfr = res["n_frames"][i]
    st = res["status"][i, :nfr]
    parts = [name, str(nfr)]
    for q in range(n):
        sf = sb = 0.0
        cnt = 0
        for j in range(nfr):
            if st[j] == 0 and res["n_formants"][i, j] > q:
                sf += res["formants"][i, j, q, 0]
                sb += res["formants"][i, j, q, 1]
                cnt += 1
        parts += [_fmt(sf / cnt if cnt else np.nan), _fmt(sb / cnt if cnt else np.nan)]
    status = 0
    for s in st:
        status |= int(s)
    return " ".join(parts + [str(status)])


@pytest.mark.parametrize("header", [44, 72])
def test_cli_lines_equal_the_engine(engine, tmp_path, header):
    runs = [(["-d", "1", "-j", "1"], ["-v", "a"], 22050),
            (["-r", "44100", "-d", "1", "-f", "100"], ["-v", "i"], 44100),
            (["-r", "16000", "-d", "0.5", "-f", "150", "-g", "160"], ["-v", "u", "-n", "20"], 16000)]
    files = [_pipeline(tmp_path, "s%d" % k, fa, va, 11 + k, header) for k, (fa, va, _) in enumerate(runs)]
    env = dict(os.environ, VS_WAV_HEADER=str(header))
    for args, kw in ((["-n", "4"], dict(n_formants=4)),
                     (["-o", "18", "-w", "30", "-t", "5", "-p", "-r"],
                      dict(order=18, window_s=0.030, hop_s=0.005, pre_emphasis=1, window="rectangular"))):
        r = subprocess.run([os.path.join(BIN, "formants")] + args + files, cwd=tmp_path, capture_output=True, text=True,
                           env=env)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        n = kw.get("n_formants", 5)
        assert lines[0] == "# file frames " + " ".join("F%d_Hz B%d_Hz" % (q, q) for q in range(1, n + 1)) + " status"
        assert len(lines) == 1 + len(files)
        for f, run, line in zip(files, runs, lines[1:]):
            x, fs = _read(tmp_path / f, header)[0], run[2]
            res = engine.lpc(x[None, :], fs, **kw)
            assert line == _cli_line(f, res, 0, n)


def test_cli_centre_coefficients_round_trip_and_bad_files(engine, tmp_path):
    good = _pipeline(tmp_path, "g", ["-d", "1", "-j", "1"], ["-v", "a"], 5)
    x, fs = _read(tmp_path / good, 44)
    open(tmp_path / "trunc.wav", "wb").write(open(tmp_path / good, "rb").read()[:30])
    raw = bytearray(open(tmp_path / good, "rb").read())
    raw[20:22] = struct.pack("<H", 3)
    open(tmp_path / "tag3.wav", "wb").write(bytes(raw))
    r = subprocess.run([os.path.join(BIN, "formants"), "-c", "-f", "-o", "30", "trunc.wav", good, "tag3.wav"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2
    assert "trunc.wav" in r.stderr and "tag3.wav" in r.stderr
    lines = r.stdout.splitlines()
    res = engine.lpc(x[None, :], fs, coefs=True, order=30, hop_s=0)
    assert lines[1] == _cli_line(good, res, 0, 5)
    assert lines[2].startswith("# frame %s 0 %d 0" % (good, res["start"][0, 0]))
    assert lines[3].startswith("# coefs %s:" % good)
    A = np.array([float(t) for t in lines[3].split(":")[1].split()])
    assert A.shape == (31,) and np.array_equal(A, res["coefs"][0, 0])
    r = subprocess.run([os.path.join(BIN, "formants"), "-o", "99", good], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1
